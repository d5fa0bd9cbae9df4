"""Host-side checks of ``nlbac_amd.ode_grid.odeint_grid``: foreign modules, bad time grids, dopri5, shapes, dtypes and
devices are refused, each with its named error, before anything touches a device (no GPU needed)."""
import pytest
import torch


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


GRID = [0.0, 0.02, 0.05, 0.055, 0.1, 0.12]


def test_odeint_grid_refuses_foreign_modules():
    from nlbac_amd.ode_grid import odeint_grid
    with pytest.raises(TypeError):
        odeint_grid(torch.nn.Linear(5, 5), torch.zeros(4, 5), GRID)


@pytest.mark.parametrize("kind,width", [("affine", 5), ("concat", 12)])
def test_odeint_grid_validates_before_touching_a_device(kind, width, monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_grid import odeint_grid
    m = model(kind)

    def no_device(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(type(m), "refresh_device_weights", no_device)
    monkeypatch.setattr(type(m), "device_handles", no_device)
    y0 = torch.zeros(4, width)
    nan, inf = float("nan"), float("inf")
    bad = [
        (ValueError, dict(t=[0.0])),                                   # T < 2
        (ValueError, dict(t=[])),
        (ValueError, dict(t=torch.zeros(2, 3))),                       # not 1-D
        (ValueError, dict(t=[0.0, 0.02, 0.02, 0.05])),                 # a repeated point
        (ValueError, dict(t=[0.0, 0.05, 0.02, 0.1])),                  # not monotone
        (ValueError, dict(t=[0.1, 0.05, 0.0])),                        # decreasing: out of scope
        (ValueError, dict(t=[0.0, nan, 0.1])),
        (ValueError, dict(t=[0.0, 0.02, inf])),
        (ValueError, dict(t=torch.tensor([0.0, 1e-50], dtype=torch.float64))),     # an interval that is 0 in float32
        (NotImplementedError, dict(method="dopri5")),
        (ValueError, dict(method="adams")),
        (ValueError, dict(y0=torch.zeros(4, width + 1))),
        (ValueError, dict(y0=torch.zeros(4, width - 1))),
        (ValueError, dict(y0=torch.zeros(width))),
        (ValueError, dict(y0=torch.zeros(0, width))),
        (TypeError, dict(y0=torch.zeros(4, width, dtype=torch.float64))),
        (TypeError, dict(y0=[[0.0] * width])),
        (ValueError, dict()),             # a CPU tensor: a CUDA device is required
    ]
    for exc, kw in bad:
        args = dict(y0=y0, t=GRID, method="rk4")
        args.update(kw)
        with pytest.raises(exc):
            odeint_grid(m, args["y0"], args["t"], method=args["method"])


def test_messages_name_what_is_out_of_scope():
    from nlbac_amd.ode_grid import odeint_grid
    m = model("affine")
    y0 = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="decreasing.*out of scope"):
        odeint_grid(m, y0, [0.1, 0.05, 0.0])
    with pytest.raises(NotImplementedError, match="one adaptive solve|ONE adaptive solve"):
        odeint_grid(m, y0, GRID, method="dopri5")


def test_steps_are_formed_as_odeint_forms_them():
    """float(t[k+1]) - float(t[k]) in Python floats, then rounded once to the C float argument."""
    import ctypes
    from nlbac_amd import ode_grid
    for t in (GRID, torch.tensor(GRID), torch.tensor(GRID, dtype=torch.float64), [k / 32 for k in range(9)]):
        tt = torch.as_tensor(t)
        want = tuple(ctypes.c_float(float(tt[k + 1]) - float(tt[k])).value for k in range(len(tt) - 1))
        assert ode_grid._steps_of(t) == want
    assert ode_grid._steps_of([k / 32 for k in range(9)]) == (1 / 32,) * 8


def test_exports_and_header_declare_the_grid_functions():
    import os
    import re
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "nlbac_hip.h")).read(), flags=re.S)
    for name in ("nlbac_node_rk_grid_fwd", "nlbac_node_rk_grid_bwd", "nlbac_concat_rk_grid_fwd", "nlbac_concat_rk_grid_bwd"):
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
        assert "const float *hs," in proto and "const float *hs_host" in proto
