"""Host-side checks of ``nlbac_amd.ode_dense.odeint_dense`` (no GPU needed): every refused argument raises its named
error before anything touches a device, the new entry points are declared in the header and in the binding's table,
and the CPU reference the GPU tests compare against (``dense_common``) pins itself — to ``O.odeint`` at its last point
and to the step sequences its two cases were chosen for."""
import os
import re

import numpy as np
import pytest
import torch

import dense_common as D
from oracle import nlbac_oracle as O

GRID = [0.0, 0.01, 0.02, 0.05, 0.3]
NEW = ("nlbac_dopri_dense_fwd", "nlbac_dopri_dense_bwd", "nlbac_dopri_dense_carry")


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


def test_odeint_dense_refuses_foreign_modules():
    from nlbac_amd.ode_dense import odeint_dense
    with pytest.raises(TypeError):
        odeint_dense(torch.nn.Linear(5, 5), torch.zeros(4, 5), GRID)


@pytest.mark.parametrize("kind,width", [("affine", 5), ("concat", 12)])
def test_odeint_dense_validates_before_touching_a_device(kind, width, monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_dense import odeint_dense
    m = model(kind)

    def no_device(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(type(m), "refresh_device_weights", no_device)
    monkeypatch.setattr(type(m), "device_handles", no_device)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", no_device)
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
        (TypeError, dict(t=torch.tensor([False, True]))),
        (ValueError, dict(atol=0.0)),
        (ValueError, dict(atol=-1e-7)),
        (ValueError, dict(atol=nan)),
        (ValueError, dict(rtol=0.0)),
        (ValueError, dict(rtol=inf)),
        (TypeError, dict(rtol="1e-5")),
        (TypeError, dict(atol=True)),
        (TypeError, dict(atol=torch.tensor(1e-7))),
        (NotImplementedError, dict(adjoint=True)),
        (ValueError, dict(y0=torch.zeros(4, width + 1))),
        (ValueError, dict(y0=torch.zeros(4, width - 1))),
        (ValueError, dict(y0=torch.zeros(width))),
        (ValueError, dict(y0=torch.zeros(0, width))),
        (TypeError, dict(y0=torch.zeros(4, width, dtype=torch.float64))),
        (TypeError, dict(y0=[[0.0] * width])),
        (ValueError, dict()),             # a CPU tensor: a CUDA device is required
    ]
    for exc, kw in bad:
        args = dict(y0=y0, t=GRID)
        args.update(kw)
        with pytest.raises(exc):
            odeint_dense(m, args.pop("y0"), args.pop("t"), **args)
    with pytest.raises(TypeError):
        odeint_dense(m, y0, GRID, method="rk4")                        # the method is dopri5: no such keyword


def test_messages_name_what_is_out_of_scope():
    from nlbac_amd.ode_dense import odeint_dense
    from nlbac_amd.ode_grid import odeint_grid
    m = model("affine")
    y0 = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="odeint_dense.*decreasing.*out of scope"):
        odeint_dense(m, y0, [0.1, 0.05, 0.0])
    with pytest.raises(NotImplementedError, match="adjoint"):
        odeint_dense(m, y0, GRID, adjoint=True)
    with pytest.raises(NotImplementedError, match="odeint_dense"):      # the grid entry points at the dense one
        odeint_grid(m, y0, GRID, method="dopri5")


def test_output_times_are_formed_as_odeint_forms_its_dt():
    """float(t[j]) - float(t[0]) of the float32 entries: a Python sequence is rounded to float32 first, as ``odeint``'s
    ``torch.as_tensor(t)`` rounds it."""
    from nlbac_amd import ode_dense
    t32 = torch.tensor([0.1, 0.3, 0.6])
    assert float(t32[2]) != 0.6           # (what the rounding is about)
    for t in ([0.1, 0.3, 0.6], t32, t32.double(), (0.1, 0.3, 0.6)):
        tt = torch.as_tensor(t)
        assert ode_dense._taus(t) == tuple(float(tt[j]) - float(tt[0]) for j in (1, 2))
        assert ode_dense._taus(t) == ode_dense._taus(t32)
    t64 = torch.tensor([0.1, 0.3, 0.6], dtype=torch.float64)
    assert ode_dense._taus(t64) == (0.3 - 0.1, 0.6 - 0.1)      # a float64 tensor's entries are taken as they are


def test_exports_and_header_declare_the_dense_functions():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    assert re.search(r"#define NLBAC_ABI_VERSION 17\b", raw) and _lib.ABI_VERSION == 17
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
    for name in NEW[:2]:
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        for arg in ("long slot_floats", "const double *ctl", "const double *hslots", "int n_slots", "const double *tau",
                    "int n_out"):
            assert arg in proto, (name, arg)


@pytest.mark.parametrize("name", ["unicycle", "cars"])
def test_reference_ends_where_the_oracles_odeint_ends(name):
    """One solve read at its last output time IS ``O.odeint`` over [t0, t_last] — same controller arithmetic, same
    interpolant — when the times are float() of the float32 entries."""
    c = D.case(name)
    times = D.times_of(c["t"])
    sd = {k: torch.tensor(v) for k, v in c["W"].items()}
    node = D.CASES[name]["node"](sd)
    info = {}
    with torch.no_grad():
        want = O.odeint(node, c["y0"], torch.tensor([times[0], times[-1]], dtype=torch.float64), method="dopri5",
                        info=info)[-1]
        two, steps2, _ = D.dense_reference(node, c["y0"], [times[0], times[-1]])
    assert torch.equal(c["out"][-1], want)
    assert torch.equal(two[-1], want) and steps2 == info["steps"] == c["steps"]
    assert torch.equal(c["out"][0], c["y0"])


@pytest.mark.parametrize("name", ["unicycle", "cars"])
def test_cases_take_the_step_sequences_they_were_chosen_for(name):
    """Several accepted steps, none rejected; steps that hold two or three outputs, one that holds none, and a last step
    that overshoots the last output; no output time near a step's end (where fp32 noise in a step size could move an
    output into the neighbouring step)."""
    c = D.case(name)
    times = D.times_of(c["t"])
    taus = [v - times[0] for v in times[1:]]
    assert all(s[2] for s in c["steps"]), c["steps"]
    assert max(s[1] for s in c["steps"]) <= (0.58 if name == "unicycle" else 0.085)
    # (later step sizes follow 0.9 ratio^-0.2 of an error ratio that is cancellation noise at the 1e-3 level: the ends
    #  move in the fourth digit from one CPU to another — test_solver_gpu's bar on step sizes)
    assert len(c["ends"]) == len(c["want_ends"])
    np.testing.assert_allclose(c["ends"], c["want_ends"], rtol=2e-3)
    assert D.outputs_per_step(c["ends"], times) == c["want_per_step"]
    assert c["ends"][-1] > taus[-1]
    assert min(abs(e - x) for e in c["ends"] for x in taus) > 2e-3 * taus[-1]
    # the fp32 reference against its fp64 twin: far below the 1e-4 bar the device is held to
    err = float((c["out"].double() - c["out64"]).abs().max() / c["out"].abs().max())
    assert err <= 1e-5, err
