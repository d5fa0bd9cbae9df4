"""Host-side checks of ``rollout(..., adjoint=True)`` / ``odeint_grid(..., adjoint=True)``: the ``adjoint_chunk`` rules,
every refusal before anything touches a device, the per-interval backward step lists (``ode_grid._sub_grid`` over
[0, length], applied from the interval's upper end), how a backward is cut into runs, and the new entry points'
declarations (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch


def f32(v):
    return ctypes.c_float(v).value


def model(kind="affine"):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


class Reached(Exception):
    pass


@pytest.mark.parametrize("chunk", [0, -1, 1.5, True])
@pytest.mark.parametrize("api", ["rollout", "odeint_grid"])
def test_adjoint_chunk_is_a_positive_int_or_none(api, chunk):
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="adjoint_chunk"):
        if api == "rollout":
            rollout(m, torch.zeros(4, 3), torch.zeros(2, 4, 2), 0.01, method="rk4", adjoint=True, adjoint_chunk=chunk)
        else:
            odeint_grid(m, torch.zeros(4, 5), [0.0, 0.1, 0.3], method="rk4", adjoint=True, adjoint_chunk=chunk)


@pytest.mark.parametrize("api", ["rollout", "odeint_grid"])
def test_adjoint_chunk_goes_with_adjoint_only(api):
    from nlbac_amd import ode_grid as G, rollout as R
    m = model()
    with pytest.raises(ValueError, match="adjoint=True"):
        if api == "rollout":
            R.rollout(m, torch.zeros(4, 3), torch.zeros(2, 4, 2), 0.01, method="rk4", adjoint_chunk=2)
        else:
            G.odeint_grid(m, torch.zeros(4, 5), [0.0, 0.1, 0.3], method="rk4", adjoint_chunk=2)


def test_rollout_dopri5_has_no_chunks():
    from nlbac_amd import rollout as R
    m = model()
    with pytest.raises(ValueError, match="dopri5"):
        R.rollout(m, torch.zeros(4, 3), torch.zeros(2, 4, 2), 0.01, method="dopri5", adjoint=True, adjoint_chunk=1)


def test_grid_dopri5_stays_not_implemented():
    from nlbac_amd.ode_grid import odeint_grid
    with pytest.raises(NotImplementedError):
        odeint_grid(model(), torch.zeros(4, 5), [0.0, 0.1, 0.3], method="dopri5", adjoint=True)


def test_odeint_adjoint_itself_is_unchanged():
    from nlbac_amd.odeint import odeint_adjoint
    m = model()
    with pytest.raises(NotImplementedError, match="step_size is not offered"):
        odeint_adjoint(m, torch.zeros(4, 5), torch.tensor([0.0, 0.01]), method="rk4", options=dict(step_size=0.004))
    with pytest.raises(NotImplementedError, match="time points"):
        odeint_adjoint(m, torch.zeros(4, 5), torch.tensor([0.0, 0.01, 0.02]), method="rk4")


def _plan_of_rollout(monkeypatch, dt, s, H=2, **kw):
    from nlbac_amd import ode_traj, rollout as R
    from test_rollout_substep_host import past_the_device_check
    m = model()
    seen = {}

    def solve_adjoint(func, iv, method, mode, one_launch, plan, x0, u, xs, *tol):
        seen.update(iv=iv, plan=plan, mode=mode)
        raise Reached

    monkeypatch.setattr(ode_traj, "solve_adjoint", solve_adjoint)
    monkeypatch.setattr(ode_traj, "solve", lambda *a, **k: pytest.fail("adjoint=True must not take the direct solve"))
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_one_launch_ok", lambda func, method: False)
    past_the_device_check(monkeypatch, R)
    with pytest.raises(Reached):
        R.rollout(m, torch.zeros(4, 3), torch.zeros(H, 4, 2), dt, method="rk4", step_size=s, adjoint=True, **kw)
    return seen


def test_backward_step_list_is_the_sub_grid_from_the_upper_end(monkeypatch):
    """step_size = 0.004 over dt = 0.01: every control interval is solved backwards in (0.004, 0.004, cut), applied in
    that order from its upper end — in the run a launch walks last to first, the cut step is each interval's lowest."""
    from nlbac_amd import ode_traj
    from nlbac_amd.ode_grid import _sub_grid
    seen = _plan_of_rollout(monkeypatch, 0.01, 0.004, adjoint_chunk=1)
    plan, iv = seen["plan"], seen["iv"]
    hs = _sub_grid(torch.tensor([0.0, 0.01], dtype=torch.float32), 0.004)[1]
    assert len(hs) == 3 and hs[0] == hs[1] == f32(0.004) and 0 < hs[2] < hs[0]
    assert abs(sum(hs) - f32(0.01)) < 1e-9
    assert type(iv) is ode_traj.HeldSteps and iv.hs == hs             # (the forward: today's held-control solve)
    assert plan.steps == (hs, hs) and plan.stacked and plan.sub and plan.chunk == 1 and plan.H == 2
    run_hs, begin = plan.run(0, 2)
    assert run_hs == [hs[2], hs[1], hs[0]] * 2 and begin == [-1, -1, 0, -1, -1, 1]
    # walked last to first: the interval's marker first, then its steps in the list's order
    walked = list(zip(reversed(run_hs), reversed(begin)))
    assert walked[:3] == [(hs[0], 1), (hs[1], -1), (hs[2], -1)]


def test_no_step_size_is_one_step_per_interval(monkeypatch):
    from nlbac_amd import ode_traj
    seen = _plan_of_rollout(monkeypatch, 0.05, None, H=3)
    plan = seen["plan"]
    assert type(seen["iv"]) is ode_traj.EqualSteps
    assert plan.steps == ((f32(0.05),),) * 3 and not plan.sub and plan.chunk is None
    assert plan.run(1, 3) == ([f32(0.05)] * 2, [1, 2])


def test_grid_intervals_get_their_own_fine_grids():
    from nlbac_amd.ode_grid import _adjoint_steps, _steps_of, _sub_grid
    t = [0.0, 0.01, 0.013, 0.03]
    assert _adjoint_steps(t, None) == [(h,) for h in _steps_of(t)]
    steps = _adjoint_steps(t, 0.004)
    assert [len(s) for s in steps] == [3, 1, 5]
    for (a, b), s in zip(zip(t, t[1:]), steps):
        assert s == _sub_grid([0.0, b - a], 0.004)[1]
        assert all(h == f32(0.004) for h in s[:-1]) and 0 < s[-1] <= f32(0.004)


def test_runs_and_chunk_choice():
    from nlbac_amd.ode_traj import AdjointPlan, _dw_rows_limit
    plan = AdjointPlan([(0.1,)] * 5, True)
    assert plan.runs(5) == [(0, 5)] and plan.runs(2) == [(3, 5), (1, 3), (0, 1)] and plan.runs(1) == [(k, k + 1) for k in (4, 3, 2, 1, 0)]
    assert plan.pick_chunk(2 ** 31, 96, 4) == 5
    assert AdjointPlan([(0.1,)] * 5, True, chunk=2).pick_chunk(2 ** 31, 96, 4) == 2
    assert AdjointPlan([(0.1,)] * 5, True, chunk=9).pick_chunk(2 ** 31, 96, 4) == 5
    # H = 16, m = 4, rk4, 32768 rows: 2^23 stage rows, which the weight-gradient launch refuses at width 64 and 100
    held = AdjointPlan([(0.005,) * 4] * 16, True)
    for hid in (64, 100):
        limit = _dw_rows_limit(hid, 64)
        assert 16 * 4 * 4 * 32768 >= limit
        chunk = held.pick_chunk(limit, 32768, 4)
        assert 1 <= chunk < 16
        assert all((hi - lo) * 4 * 4 * 32768 < limit for lo, hi in held.runs(chunk))
        assert any((hi - lo + 1) * 4 * 4 * 32768 >= limit for lo, hi in held.runs(chunk))


def test_exports_and_header_declare_the_adjoint_trajectory_functions():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define NLBAC_ABI_VERSION 17\b", raw) and _lib.ABI_VERSION == 17
    for name in ("nlbac_node_adj_traj", "nlbac_node_adj_traj_ok", "nlbac_concat_adj_traj", "nlbac_concat_adj_traj_ok"):
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
    flat = " ".join(re.search(r"int nlbac_node_adj_traj\s*\((.*?)\);", txt, flags=re.S).group(1).split())
    for arg in ("const float *hs, const float *hs_host,", "const int *begin, const int *begin_host,", "float *carry, int top,"):
        assert arg in flat, arg
