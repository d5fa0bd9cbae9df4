"""Host-side checks of ``rollout(..., step_size=s)``: the fine steps of a control interval are what ``ode_grid._sub_grid``
builds for ``[0, dt]``, every refusal comes before anything touches a device, ``step_size=None`` is the path as it was,
and the four ``*_hold_*`` entry points are declared (no GPU needed)."""
import ctypes

import pytest
import torch


def f32(v):
    return ctypes.c_float(v).value


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


class Reached(Exception):
    pass


SCHEDULES = [
    (0.05, 0.02, (0.019999999552965164, 0.019999999552965164, 0.010000000707805157)),
    (1 / 8, 1 / 32, (1 / 32,) * 4),
    (0.02, 0.003, None),
    (0.02, 0.02, None),
    (0.02, 1.0, None),
]
M_OF = {(0.05, 0.02): 3, (1 / 8, 1 / 32): 4, (0.02, 0.003): 7, (0.02, 0.02): 1, (0.02, 1.0): 1}


@pytest.mark.parametrize("dt,s,steps", SCHEDULES)
def test_schedule_is_sub_grids(dt, s, steps, monkeypatch):
    """What reaches the solve: HeldSteps with the m fine steps ``_sub_grid(tensor([0, dt], float32), s)`` returns."""
    from nlbac_amd import ode_traj, rollout as R
    from nlbac_amd.ode_grid import _sub_grid
    taus, hs, ofs, theta = _sub_grid(torch.tensor([0.0, dt], dtype=torch.float32), s)
    assert theta == (1.0,) and len(hs) == M_OF[(dt, s)] and ofs[-1] == 2
    assert all(h == f32(h) and h > 0 for h in hs)
    if steps is not None:
        assert hs == steps
    if len(hs) == 1:
        assert hs == (f32(dt),)
    seen = {}

    def solve(func, iv, method, mode, one_launch, x0, u, xs, *tol):
        seen["iv"] = iv
        raise Reached

    m = model("affine")
    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_one_launch_ok", lambda func, method: False)
    past_the_device_check(monkeypatch, R)
    H = 5
    with pytest.raises(Reached):
        R.rollout(m, torch.zeros(4, 3), torch.zeros(H, 4, 2), dt, method="euler", step_size=s)
    iv = seen["iv"]
    assert type(iv) is ode_traj.HeldSteps
    assert iv.hs == hs and iv.m == len(hs) and iv.H == H * len(hs) and iv.n_out == H and iv.launch_H == H
    assert (iv.api, iv.infix) == ("rollout", "hold")
    assert iv.solvers_key not in (ode_traj.EqualSteps.solvers_key, ode_traj.GridSteps.solvers_key,
                                  ode_traj.SubGridSteps.solvers_key)
    assert iv.du_shape(4, 2) == (H, 4, 2)
    u = list(range(H))
    assert [iv.control(u, i) for i in range(iv.H)] == [i // iv.m for i in range(iv.H)]
    assert [iv.step(i) for i in range(iv.H)] == list(hs) * H


def past_the_device_check(monkeypatch, R):
    """``rollout._check`` with its last check, the one for a CUDA device, let through: the way to the solve without a GPU."""
    real = R._check

    def check(func, x0, controls, dt, method, step_size=None):
        try:
            return real(func, x0, controls, dt, method, step_size)
        except ValueError as e:
            if "CUDA" not in str(e):
                raise
        # (what it returns behind that check comes from the same rule)
        from nlbac_amd.ode_grid import _sub_grid
        grid = torch.tensor([0.0, float(dt)], dtype=torch.float32)
        return float(grid[1]), (None if step_size is None else _sub_grid(grid, step_size)[1])
    monkeypatch.setattr(R, "_check", check)


def test_held_steps_hooks_follow_the_kernel_order():
    """The chained path's torch-side hooks on CPU tensors: outputs and their gradients meet the fine intervals at
    r = m-1 only, du is summed inside a control interval from r = m-1 down and stacked per control interval."""
    from nlbac_amd.ode_traj import HeldSteps
    iv = HeldSteps((0.25, 0.25, 0.125), 2, "cpu")
    assert (iv.H, iv.m, iv.n_out) == (6, 3, 2)
    xs = torch.zeros(2, 1, 1)
    for i in range(6):
        x = iv.emit(xs, i, None, torch.full((1, 1), float(i + 1)))
        assert float(x) == i + 1
    assert xs.flatten().tolist() == [3.0, 6.0]
    dout = torch.tensor([10.0, 20.0, 30.0]).view(3, 1, 1)
    c = torch.full((1, 1), 0.5)
    assert float(iv.grad_in(dout, 5, None)) == 30.0
    assert float(iv.grad_in(dout, 4, c)) == 0.5 and float(iv.grad_in(dout, 3, c)) == 0.5
    assert float(iv.grad_in(dout, 2, c)) == 20.5
    assert float(iv.grad_carry(dout, 3, c)) == 0.5
    acc = None
    for i in range(5, -1, -1):
        acc = iv.add_du(acc, i, torch.full((1, 1), 2.0 ** i))
    assert acc.shape == (2, 1, 1) and acc.flatten().tolist() == [1.0 + 2.0 + 4.0, 8.0 + 16.0 + 32.0]


@pytest.mark.parametrize("kind,ns,nc", [("affine", 3, 2), ("concat", 10, 2)])
def test_step_size_validates_before_touching_a_device(kind, ns, nc, monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.rollout import rollout
    m = model(kind)
    assert (m.n_s, m.n_u if m.affine else m.n_carry) == (ns, nc)

    def no_device(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(type(m), "refresh_device_weights", no_device)
    monkeypatch.setattr(type(m), "device_handles", no_device)
    B, H = 4, 3
    x0, c = torch.zeros(B, ns), torch.zeros(H, B, nc)
    nan, inf = float("nan"), float("inf")
    bad = [
        (ValueError, dict(step_size=0.0)),
        (ValueError, dict(step_size=0)),
        (ValueError, dict(step_size=-0.01)),
        (ValueError, dict(step_size=nan)),
        (ValueError, dict(step_size=inf)),
        (ValueError, dict(step_size=-inf)),
        (ValueError, dict(step_size=1e-12)),               # 2^31 fine intervals or more
        (TypeError, dict(step_size=True)),
        (TypeError, dict(step_size="0.01")),
        (TypeError, dict(step_size=[0.01])),
        (TypeError, dict(step_size=torch.tensor(0.01))),
        (TypeError, dict(step_size=1j)),
        (ValueError, dict(method="adams")),
        (ValueError, dict(dt=0.0)),
        (ValueError, dict(dt=nan)),
        (TypeError, dict(dt=True)),
        (TypeError, dict(dt=torch.tensor(0.05))),
        (ValueError, dict(x0=torch.zeros(B, ns + 1))),
        (ValueError, dict(x0=torch.zeros(B))),
        (ValueError, dict(x0=torch.zeros(0, ns), controls=torch.zeros(H, 0, nc))),
        (TypeError, dict(x0=torch.zeros(B, ns, dtype=torch.float64))),
        (TypeError, dict(x0=[[0.0] * ns] * B)),
        (ValueError, dict(controls=torch.zeros(H, B, nc + 1))),
        (ValueError, dict(controls=torch.zeros(H, B + 1, nc))),
        (ValueError, dict(controls=torch.zeros(0, B, nc))),
        (ValueError, dict(controls=torch.zeros(B, nc))),
        (TypeError, dict(controls=torch.zeros(H, B, nc, dtype=torch.float64))),
        (TypeError, dict(controls=None)),
    ]
    for exc, kw in bad:
        args = dict(x0=x0, controls=c, dt=0.05, method="rk4", step_size=0.02)
        args.update(kw)
        with pytest.raises(exc):
            rollout(m, args["x0"], args["controls"], args["dt"], method=args["method"], step_size=args["step_size"])
    with pytest.raises(TypeError):
        rollout(torch.nn.Linear(3, 3), x0, c, 0.05, method="rk4", step_size=0.02)

    # dopri5 does not take the option (torchdiffeq ignores it there; this build says so), whatever its value
    for s in (0.02, -1.0, "x"):
        with pytest.raises(ValueError, match="dopri5"):
            rollout(m, x0, c, 0.05, method="dopri5", step_size=s)

    # H * m * stages * B at the launcher's limit, rows that take no memory: 4 x 7 x 4 stages x 2^25 rows = 7 * 2^29
    big = 2 ** 25
    xb, cb = x0[:1].expand(big, ns), c[:1, :1].expand(4, big, nc)
    with pytest.raises(ValueError, match=r"2\^31"):
        rollout(m, xb, cb, 0.02, method="rk4", step_size=0.003)
    # (below the limit the same call gets as far as the device check: 4 x 1 x 1 stage x 2^25 rows = 2^27)
    with pytest.raises(ValueError, match="CUDA"):
        rollout(m, xb, cb, 0.02, method="euler", step_size=0.02)

    # everything passed: the CPU tensor is what stops it, last
    for method in ("euler", "rk4"):
        for s in (0.02, 0.003, 1.0, 1):
            with pytest.raises(ValueError, match="CUDA"):
                rollout(m, x0, c, 0.05, method=method, step_size=s)
    with pytest.raises(ValueError, match="CUDA"):
        rollout(m, x0, c, 0.05, method="dopri5")            # (and without step_size dopri5 is served as before)


@pytest.mark.parametrize("method", ["euler", "rk4", "dopri5"])
def test_no_step_size_is_the_path_as_it_was(method, monkeypatch):
    from nlbac_amd import ode_traj, rollout as R
    m = model("affine")
    seen = {}

    def solve(func, iv, meth, mode, one_launch, x0, u, xs, *tol):
        seen.update(iv=iv, method=meth, tol=tol, xs=tuple(xs.shape))
        raise Reached

    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_one_launch_ok", lambda func, method: False)
    past_the_device_check(monkeypatch, R)
    for kw in (dict(), dict(step_size=None)):
        seen.clear()
        with pytest.raises(Reached):
            R.rollout(m, torch.zeros(4, 3), torch.zeros(5, 4, 2), 0.05, method=method, **kw)
        iv = seen["iv"]
        assert type(iv) is ode_traj.EqualSteps and iv.H == 5 and iv.launch_H == 5 and iv.n_out == 5
        assert iv.dt == f32(0.05) and iv.step_args() == (f32(0.05),)
        assert seen["method"] == method and seen["tol"] == (1e-7, 1e-5) and seen["xs"] == (5, 4, 3)


def test_exports_and_header_declare_the_hold_functions():
    import os
    import re
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define NLBAC_ABI_VERSION 17\b", raw) and _lib.ABI_VERSION == 17
    for name in ("nlbac_node_rk_hold_fwd", "nlbac_node_rk_hold_bwd", "nlbac_concat_rk_hold_fwd",
                 "nlbac_concat_rk_hold_bwd"):
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
        sib = name.replace("_hold_", "_grid_")
        grid = re.search(r"int %s\s*\((.*?)\);" % sib, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(grid.split(",")) + 1           # int m
        flat = " ".join(proto.split())
        for arg in ("const float *hs,", "const float *hs_host, int m,"):
            assert arg in flat, (name, arg)
        # the binding: the sibling's argument types with one int behind hs_host
        at = [i for i, t in enumerate(_lib._PROTOS[sib]) if t is _lib.c_float_p][2] + 1      # (beta, c_out, hs_host)
        assert _lib._PROTOS[name] == _lib._PROTOS[sib][:at] + [ctypes.c_int] + _lib._PROTOS[sib][at:], name
