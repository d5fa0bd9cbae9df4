"""Host-side checks of ``odeint_grid(..., step_size=s)`` and ``odeint(..., options=dict(step_size=s))``: the fine grid
and the placement of the output points (``ode_grid._sub_grid``) against a restatement of torchdiffeq 0.2.3's rule, every
refusal before anything touches a device, and the four ``*_subgrid_*`` entry points' declarations (no GPU needed)."""
import ctypes
import math

import pytest
import torch

G2 = [0, 1 / 32, 3 / 32, 4 / 32, 8 / 32]
GRID = [0.0, 0.02, 0.05, 0.055, 0.1, 0.12]


def f32(v):
    return ctypes.c_float(v).value


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


def rule(t, s):
    """torchdiffeq 0.2.3: ``_grid_constructor_from_step_size`` (arange(niters) * s + t[0], last point replaced by t[-1])
    and the ``integrate`` loop of the fixed-grid solvers with ``_linear_interp`` — restated, in Python floats."""
    t = [float(v) for v in t]
    niters = math.ceil((t[-1] - t[0]) / s + 1)
    tau = [i * s + t[0] for i in range(niters)]
    tau[-1] = t[-1]
    hs = [f32(tau[i + 1] - tau[i]) for i in range(niters - 1)]
    where, theta, j = {}, [], 1
    for i in range(niters - 1):
        while j < len(t) and tau[i + 1] >= t[j]:
            where[j] = i
            if t[j] == tau[i + 1]:
                theta.append(1.0)
            elif t[j] == tau[i]:
                theta.append(0.0)
            else:
                theta.append(f32((t[j] - tau[i]) / (tau[i + 1] - tau[i])))
            j += 1
    ofs = [1 + sum(1 for jj in where if where[jj] < i) for i in range(niters)]
    return tuple(tau), tuple(hs), tuple(ofs), tuple(theta)


CASES = [(GRID, 0.03), (GRID, 0.2), (GRID, 0.12), (GRID, 0.007), (GRID, 0.01), (G2, 1 / 32), (G2, 1 / 64), (G2, 3 / 64)]


@pytest.mark.parametrize("t,s", CASES)
def test_sub_grid_follows_the_rule(t, s):
    from nlbac_amd import ode_grid
    for tt in (t, torch.tensor(t, dtype=torch.float64)):
        got = ode_grid._sub_grid(tt, s)
        assert got == rule(t, s)
        taus, hs, ofs, theta = got
        N = len(hs)
        assert len(taus) == N + 1 and len(ofs) == N + 1 and len(theta) == len(t) - 1
        assert taus[0] == t[0] and taus[-1] == t[-1]
        assert ofs[0] == 1 and ofs[-1] == len(t) and all(a <= b for a, b in zip(ofs, ofs[1:]))
        assert all(h > 0 and h == f32(h) for h in hs) and all(0.0 <= th <= 1.0 for th in theta)


def test_sub_grid_named_cases():
    from nlbac_amd.ode_grid import _sub_grid
    taus, hs, ofs, theta = _sub_grid(GRID, 0.03)
    assert len(hs) == 4 and ofs == (1, 2, 4, 4, 6)          # one interval without an output, two with two each
    for s in (0.2, 0.12):
        taus, hs, ofs, theta = _sub_grid(GRID, s)
        assert len(hs) == 1 and ofs == (1, 6) and hs == (f32(0.12),) and theta[-1] == 1.0
    taus, hs, ofs, theta = _sub_grid(GRID, 0.007)
    assert len(hs) == 18 and hs[-1] == f32(0.12 - 17 * 0.007) and abs(hs[-1] - 0.001) < 1e-9
    assert _sub_grid(GRID, 0.01)[3] == (1.0, 1.0, 0.5, 1.0, 1.0)
    for s, N in ((1 / 32, 8), (1 / 64, 16)):
        taus, hs, ofs, theta = _sub_grid(G2, s)
        assert len(hs) == N and theta == (1.0,) * 4 and hs == (s,) * N
    taus, hs, ofs, theta = _sub_grid(G2, 3 / 64)
    assert theta == (f32(2 / 3), 1.0, f32(2 / 3), 1.0) and hs[-1] == 1 / 64
    assert _sub_grid(GRID, 1) == _sub_grid(GRID, 1.0)        # an int is a Python number


def test_sub_grid_refusals():
    from nlbac_amd.ode_grid import _sub_grid
    nan, inf = float("nan"), float("inf")
    for bad in (0, 0.0, -0.01, nan, inf, -inf):
        with pytest.raises(ValueError):
            _sub_grid(GRID, bad)
    for bad in (True, False, "0.01", None, [0.01], torch.tensor(0.01), 1j):
        with pytest.raises(TypeError):
            _sub_grid(GRID, bad)
    with pytest.raises(ValueError):
        _sub_grid([0.0, 0.05, 0.02], 0.01)                   # the grid's own checks hold
    with pytest.raises(ValueError):
        _sub_grid(GRID, 1e-12)                               # 2^31 fine intervals or more
    # rounding can leave a last interval that is not a positive float32: named, not solved
    # (6 * 0.1 / 0.1 is just above 6: seven fine intervals, the last one from 6 * 0.1 to 6 * 0.1)
    with pytest.raises(ValueError, match="interval 6 of 7"):
        _sub_grid([0.0, 6 * 0.1], 0.1)


@pytest.mark.parametrize("kind,width", [("affine", 5), ("concat", 12)])
def test_step_size_validates_before_touching_a_device(kind, width, monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.odeint import odeint, odeint_adjoint
    m = model(kind)

    def no_device(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(type(m), "refresh_device_weights", no_device)
    monkeypatch.setattr(type(m), "device_handles", no_device)
    y0 = torch.zeros(4, width)
    nan, inf = float("nan"), float("inf")
    bad = [
        (ValueError, dict(step_size=0.0)),
        (ValueError, dict(step_size=0)),
        (ValueError, dict(step_size=-0.01)),
        (ValueError, dict(step_size=nan)),
        (ValueError, dict(step_size=inf)),
        (TypeError, dict(step_size=True)),
        (TypeError, dict(step_size="0.01")),
        (TypeError, dict(step_size=[0.01])),
        (TypeError, dict(step_size=torch.tensor(0.01))),
        (NotImplementedError, dict(method="dopri5")),
        (NotImplementedError, dict(method="dopri5", step_size=-1.0)),     # dopri5 whatever step_size is
        (ValueError, dict(method="adams")),
        (ValueError, dict(t=[0.0, 0.05, 0.02, 0.1])),
        (ValueError, dict(t=[0.0, 6 * 0.1], step_size=0.1)),       # a degenerate last fine interval
        (ValueError, dict(step_size=1e-12)),
        (ValueError, dict(y0=torch.zeros(4, width + 1))),
        (TypeError, dict(y0=torch.zeros(4, width, dtype=torch.float64))),
        (ValueError, dict()),             # a CPU tensor: a CUDA device is required
    ]
    for exc, kw in bad:
        args = dict(y0=y0, t=GRID, method="rk4", step_size=0.03)
        args.update(kw)
        with pytest.raises(exc):
            odeint_grid(m, args["y0"], args["t"], method=args["method"], step_size=args["step_size"])

    # N * stages * B at the launcher's limit (rows that take no memory): 120 fine intervals x 4 stages x 2^23 rows
    with pytest.raises(ValueError, match=r"2\^31"):
        odeint_grid(m, y0[:1].expand(2 ** 23, width), GRID, method="rk4", step_size=0.001)

    two = [0.01, 0.03]
    # odeint: the one option is options=dict(step_size=s) under euler / rk4; everything else is refused as before
    for kw in (dict(step_size=0.004), dict(options=dict(step_size=0.004, perturb=True)), dict(options=dict(grid_constructor=None)),
               dict(options=[("step_size", 0.004)]), dict(adjoint_options=dict(step_size=0.004)),
               dict(options=dict(step_size=0.004), max_num_steps=5)):
        for fn in (odeint, odeint_adjoint):
            with pytest.raises(TypeError, match="unsupported options"):
                fn(m, y0, two, method="euler", **kw)
    with pytest.raises(ValueError, match="dopri5"):
        odeint(m, y0, two, method="dopri5", options=dict(step_size=0.004))
    with pytest.raises(ValueError, match="dopri5"):
        odeint(m, y0, two, options=dict(step_size=0.004))                 # (dopri5 is odeint's default method)
    for method in ("euler", "rk4", "dopri5"):
        with pytest.raises(NotImplementedError):
            odeint_adjoint(m, y0, two, method=method, options=dict(step_size=0.004))
    with pytest.raises(NotImplementedError, match="time points"):
        odeint(m, y0, GRID, method="rk4", options=dict(step_size=0.004))
    for exc, s in ((ValueError, 0.0), (ValueError, -1.0), (ValueError, nan), (TypeError, True), (TypeError, "x")):
        with pytest.raises(exc):
            odeint(m, y0, two, method="rk4", options=dict(step_size=s))
    with pytest.raises(ValueError, match="CUDA"):                          # everything passed: the CPU tensor is what stops it
        odeint(m, y0, two, method="rk4", options=dict(step_size=0.004))


def test_exports_and_header_declare_the_subgrid_functions():
    import os
    import re
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define NLBAC_ABI_VERSION 17\b", raw) and _lib.ABI_VERSION == 17
    for name in ("nlbac_node_rk_subgrid_fwd", "nlbac_node_rk_subgrid_bwd", "nlbac_concat_rk_subgrid_fwd",
                 "nlbac_concat_rk_subgrid_bwd"):
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
        grid = re.search(r"int %s\s*\((.*?)\);" % name.replace("_subgrid_", "_grid_"), txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(grid.split(",")) + 5           # ofs, ofs_host, theta, theta_host, T
        for arg in ("const float *hs,", "const float *hs_host", "const int *ofs,", "const int *ofs_host", "const float *theta,",
                    "const float *theta_host", "int T,"):
            assert arg in " ".join(proto.split()), (name, arg)
