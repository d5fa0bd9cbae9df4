"""Host-side checks of ``odeint_dense(..., step_control=, max_steps=, info=)`` (no GPU needed): every refusal comes
before anything touches a device — with every device entry patched to fail, as ``test_odeint_dense_host`` patches them —
``step_control="batch"`` is the call as it was, the two ``nlbac_node_dopri_tile_dense_*`` entry points are declared,
and they refuse bad arguments with a message before anything is launched."""
import os
import re

import pytest
import torch

from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)
from test_rollout_tile_host import backward_refusals, forward_refusals, tile_args

GRID = [0.0, 0.01, 0.02, 0.05, 0.3]


def model(kind="affine", **kw):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6, **kw) if kind == "affine" else NeuralODEModel(12, 10)


def y0_of(m, B=4):
    return torch.zeros(B, m.n_s + (m.n_u if m.affine else m.n_carry))


@pytest.fixture
def no_device(monkeypatch):
    """Every way to a device fails (``test_odeint_dense_host``'s regime): a check that came late shows as an
    AssertionError instead of the error it should have raised."""
    from nlbac_amd import _lib
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel

    def fail(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", fail)
    monkeypatch.setattr(_lib, "load", fail)
    monkeypatch.setattr(NeuralODEModel, "refresh_device_weights", fail)
    monkeypatch.setattr(NeuralODEModel, "device_handles", fail)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", fail)


def test_step_control_is_one_of_two_strings(no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    for bad in ("sample", "", None, 1):
        with pytest.raises(ValueError, match="step_control"):
            odeint_dense(m, y0_of(m), GRID, step_control=bad)


def test_tile_with_the_single_net_form_is_not_built(no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model("concat")
    with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
        odeint_dense(m, y0_of(m), GRID, step_control="tile")


@pytest.mark.parametrize("kw", [dict(hidden_dim=256), dict(hidden_dim=96), dict(f_depth=4), dict(g_depth=5)])
def test_tile_with_nets_the_kernels_refuse_is_not_built(kw, no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model(**kw)
    with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
        odeint_dense(m, y0_of(m), GRID, step_control="tile")


@pytest.mark.parametrize("kw", [dict(max_steps=8), dict(info={}), dict(max_steps=8, info={})])
def test_max_steps_and_info_go_with_tile(kw, no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    with pytest.raises(ValueError, match="step_control='tile'"):
        odeint_dense(m, y0_of(m), GRID, **kw)
    with pytest.raises(ValueError, match="step_control='tile'"):
        odeint_dense(m, y0_of(m), GRID, step_control="batch", **kw)


@pytest.mark.parametrize("bad", [0, -1, 5.0, "8", True])
def test_max_steps_is_an_int_of_at_least_one(bad, no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    with pytest.raises(ValueError, match="max_steps"):
        odeint_dense(m, y0_of(m), GRID, step_control="tile", max_steps=bad)


def test_max_steps_times_stages_times_rows_stays_below_2_31(no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    with pytest.raises(ValueError, match="2\\^31"):
        odeint_dense(m, y0_of(m, 4), GRID, step_control="tile", max_steps=2 ** 31 // (7 * 4) + 1)
    with pytest.raises(ValueError, match="CUDA"):          # (the largest that passes gets as far as the device check)
        odeint_dense(m, y0_of(m, 4), GRID, step_control="tile", max_steps=(2 ** 31 - 1) // (7 * 4))


@pytest.mark.parametrize("bad", [[], "info", 1])
def test_info_is_a_dict(bad, no_device):
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    with pytest.raises(ValueError, match="info"):
        odeint_dense(m, y0_of(m), GRID, step_control="tile", info=bad)


def test_the_other_checks_still_come_first_and_the_device_check_last(no_device):
    """Under ``"tile"`` the grid, the tolerances and ``y0`` are checked as they were; with everything in order a CPU
    call gets as far as the device check, and no further."""
    from nlbac_amd.ode_dense import odeint_dense
    m = model()
    y0 = y0_of(m)
    tile = dict(step_control="tile", max_steps=5, info={})
    with pytest.raises(ValueError, match="decreasing"):
        odeint_dense(m, y0, [0.1, 0.05, 0.0], **tile)
    with pytest.raises(ValueError, match="atol"):
        odeint_dense(m, y0, GRID, atol=0.0, **tile)
    with pytest.raises(NotImplementedError, match="adjoint"):
        odeint_dense(m, y0, GRID, adjoint=True, **tile)
    with pytest.raises(ValueError, match="y0 must be"):
        odeint_dense(m, torch.zeros(4, 6), GRID, **tile)
    with pytest.raises(TypeError):
        odeint_dense(torch.nn.Linear(5, 5), y0, GRID, **tile)
    with pytest.raises(ValueError, match="CUDA"):
        odeint_dense(m, y0, GRID, **tile)
    with pytest.raises(ValueError, match="CUDA"):
        odeint_dense(m, y0, GRID, step_control="tile")


class Reached(Exception):
    pass


def test_batch_is_the_call_as_it_was(monkeypatch):
    """The default call and ``step_control="batch"`` hand ``SolveNode.apply`` exactly what they handed
    ``_DenseFunction.apply``: in the batch solve's object the model, the cached solver of the keep mode, the output times,
    the tolerances and the mode; then ``y0`` and the parameters."""
    from nlbac_amd import ode_dense as OD
    m = model()
    seen = []

    class Solver:
        fused = device_loop = True

        def _chain_ok(self, P, n):
            return (P, n) == (1, 4)

    sv = Solver()

    def apply(*a):
        seen.append(a)
        raise Reached

    monkeypatch.setattr(OD.SolveNode, "apply", staticmethod(apply))
    monkeypatch.setattr(OD, "solver_of", lambda func, mode: (sv, seen.append(("solver_of", func, mode)))[0])
    monkeypatch.setattr(OD, "_check_device", lambda y0: None)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: seen.append(("refresh", self)))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(OD, "_DenseTileSolve", lambda *a: pytest.fail("the tile path was taken"))
    y0 = torch.rand(4, 5, generator=torch.Generator().manual_seed(1)).requires_grad_()
    for kw in ({}, dict(step_control="batch")):
        with pytest.raises(Reached):
            OD.odeint_dense(m, y0, GRID, atol=1e-6, rtol=1e-4, **kw)
    assert len(seen) == 6
    for k in (0, 3):
        assert seen[k] == ("solver_of", m, "params") and seen[k + 1] == ("refresh", m)
        a = seen[k + 2]
        solve = a[0]
        assert type(solve) is OD._DenseSolve and solve.func is m and solve.sv is sv and solve.taus == OD._taus(GRID)
        assert (solve.tol, solve.mode) == ((1e-6, 1e-4), "params")
        assert a[1] == 1 and a[2] is y0 and len(a) == 3 + len(list(m.parameters()))
        assert all(p is q for p, q in zip(a[3:], m.parameters()))


def test_tile_reaches_the_tile_solve_and_leaves_the_cached_solvers_alone(monkeypatch):
    from nlbac_amd import ode_dense as OD
    m = model()
    seen = []

    def apply(*a):
        seen.append(a)
        raise Reached

    monkeypatch.setattr(OD.SolveNode, "apply", staticmethod(apply))
    monkeypatch.setattr(OD, "solver_of", lambda func, mode: pytest.fail("the batch path's solvers were asked for"))
    monkeypatch.setattr(OD, "_check_device", lambda y0: None)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: pytest.fail("the tile path asks no capture state"))
    info = {}
    y0 = y0_of(m)
    for max_steps, want in ((None, 32), (7, 7), (1, 1)):
        with pytest.raises(Reached):
            OD.odeint_dense(m, y0, GRID, step_control="tile", max_steps=max_steps, info=info)
        a = seen[-1]
        solve = a[0]
        assert type(solve) is OD._DenseTileSolve and solve.func is m and solve.taus == OD._taus(GRID)
        assert (solve.tol, solve.mode) == ((1e-7, 1e-5), "params")
        assert solve.slots == want and solve.info is info and a[1] == 1 and a[2] is y0
    assert OD.SOLVERS_KEY not in m.__dict__


def test_entry_points_are_declared():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in raw
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("nlbac_node_dopri_tile_dense_fwd", "nlbac_node_dopri_tile_dense_bwd"):
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]), name
        for arg in ("int n_out", "int max_slots", "const int *ov_slot", "const float *ov_x"):
            assert arg.replace("const ", "") in proto.replace("const ", ""), (name, arg)
    src = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    assert "node_tile_dense_kernels.hip" in open(os.path.join(src, "Makefile")).read()


def test_forward_refuses_before_launching(lib):
    name = "nlbac_node_dopri_tile_dense_fwd"
    forward_refusals(lib, name)
    kw, keep = tile_args(lib, name)
    assert "bad rows / output times" in refused(lib, name, dict(kw, n_out=0), "n_out = 0")
    assert "max_slots must be at least 1" in refused(lib, name, dict(kw, max_slots=0), "no slot")
    assert "null pointer" in refused(lib, name, dict(kw, tau=None), "a null tau")


def test_backward_refuses_before_launching(lib):
    name = "nlbac_node_dopri_tile_dense_bwd"
    backward_refusals(lib, name)
    kw, keep = tile_args(lib, name)
    assert "max_slots must be at least 1" in refused(lib, name, dict(kw, max_slots=0), "no slot")
