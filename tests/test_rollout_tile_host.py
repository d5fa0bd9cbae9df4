"""Host-side checks of ``rollout(..., step_control=, max_steps=, info=)``: every refusal comes before anything touches a
device (CPU tensors reach it), ``step_control="batch"`` is the call as it was, and the three
``nlbac_node_dopri_tile_*`` entry points are declared (no GPU needed)."""
import os
import re

import pytest
import torch


def model(kind="affine", **kw):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6, **kw) if kind == "affine" else NeuralODEModel(12, 10)


def args(m, B=4, H=5):
    nc = m.n_u if m.affine else m.n_carry
    return torch.zeros(B, m.n_s), torch.zeros(H, B, nc), 0.02


def test_step_control_is_one_of_two_strings():
    from nlbac_amd.rollout import rollout
    m = model()
    for bad in ("sample", "", None, 1):
        with pytest.raises(ValueError, match="step_control"):
            rollout(m, *args(m), method="dopri5", step_control=bad)


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_tile_needs_an_adaptive_method(method):
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="fixed grid"):
        rollout(m, *args(m), method=method, step_control="tile")


def test_tile_with_the_adjoint_is_not_built():
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(NotImplementedError, match="adjoint"):
        rollout(m, *args(m), method="dopri5", step_control="tile", adjoint=True)


def test_tile_with_the_single_net_form_is_not_built():
    from nlbac_amd.rollout import rollout
    m = model("concat")
    with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
        rollout(m, *args(m), method="dopri5", step_control="tile")


@pytest.mark.parametrize("kw", [dict(hidden_dim=256), dict(hidden_dim=96), dict(f_depth=4), dict(g_depth=5)])
def test_tile_with_nets_the_kernels_refuse_is_not_built(kw):
    from nlbac_amd.rollout import rollout
    m = model(**kw)
    with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
        rollout(m, *args(m), method="dopri5", step_control="tile")


@pytest.mark.parametrize("kw", [dict(max_steps=8), dict(info={}), dict(max_steps=8, info={})])
@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_max_steps_and_info_go_with_tile(kw, method):
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="step_control='tile'"):
        rollout(m, *args(m), method=method, **kw)
    with pytest.raises(ValueError, match="step_control='tile'"):
        rollout(m, *args(m), method=method, step_control="batch", **kw)


@pytest.mark.parametrize("bad", [4, 0, -1, 5.0, "8", True])
def test_max_steps_is_an_int_of_at_least_H(bad):
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="max_steps"):
        rollout(m, *args(m, H=5), method="dopri5", step_control="tile", max_steps=bad)


def test_max_steps_times_stages_times_rows_stays_below_2_31():
    from nlbac_amd.rollout import rollout
    m = model()
    x0, c, dt = args(m, B=4, H=1)
    with pytest.raises(ValueError, match="2\\^31"):
        rollout(m, x0, c, dt, method="dopri5", step_control="tile", max_steps=2 ** 31 // (7 * 4) + 1)


def test_info_is_a_dict():
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="info"):
        rollout(m, *args(m), method="dopri5", step_control="tile", info=[])


def test_the_checks_come_before_the_device_check():
    """With everything in order a CPU call gets as far as the device check, and no further."""
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="CUDA"):
        rollout(m, *args(m), method="dopri5", step_control="tile", max_steps=5, info={})


class Reached(Exception):
    pass


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_batch_is_the_call_as_it_was(method, monkeypatch):
    """``step_control="batch"`` hands ``ode_traj.solve`` exactly what a call without the keyword hands it."""
    from nlbac_amd import ode_traj, rollout as R
    m = model()
    seen = []

    def solve(func, iv, method, mode, one_launch, x0, u, xs, *tol):
        seen.append((func, type(iv), dict(vars(iv)), method, mode, one_launch, x0.clone(), u.clone(), tuple(xs.shape), tol))
        raise Reached

    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_one_launch_ok", lambda func, method: False)
    monkeypatch.setattr(R, "_check_device", lambda x0, controls: None)
    g = torch.Generator().manual_seed(1)
    x0, c = torch.rand(4, 3, generator=g), torch.rand(5, 4, 2, generator=g).requires_grad_()
    for kw in ({}, dict(step_control="batch")):
        with pytest.raises(Reached):
            R.rollout(m, x0, c, 0.02, method=method, atol=1e-6, rtol=1e-4, **kw)
    a, b = seen
    assert a[0] is b[0] and a[1] is b[1] is ode_traj.EqualSteps and a[2] == b[2]
    assert a[3:6] == b[3:6] and a[8:] == b[8:]
    assert torch.equal(a[6], b[6]) and torch.equal(a[7], b[7])


def test_tile_reaches_the_solve_as_tile_steps(monkeypatch):
    from nlbac_amd import ode_traj, rollout as R
    m = model()
    seen = {}

    def solve(func, iv, method, mode, one_launch, x0, u, xs, *tol):
        seen.update(iv=iv, method=method, one=one_launch)
        raise Reached

    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_check_device", lambda x0, controls: None)
    info = {}
    for max_steps, want in ((None, 40), (7, 7)):
        with pytest.raises(Reached):
            R.rollout(m, *args(m, H=5), method="dopri5", step_control="tile", max_steps=max_steps, info=info)
        iv = seen["iv"]
        assert type(iv) is ode_traj.TileSteps and isinstance(iv, ode_traj.EqualSteps)
        assert (iv.H, iv.max_steps, iv.info is info, seen["method"], seen["one"]) == (5, want, True, "dopri5", True)


def test_shapes_ok_follows_the_kernels_rule():
    from nlbac_amd.ode_traj import AffineTileDopri
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    assert AffineTileDopri.shapes_ok(NeuralODEModel(3, 3, 6))
    assert AffineTileDopri.shapes_ok(NeuralODEModel(6, 6, 12))
    assert AffineTileDopri.shapes_ok(NeuralODEModel(3, 3, 6, hidden_dim=64))
    assert AffineTileDopri.shapes_ok(NeuralODEModel(3, 3, 6, hidden_dim=128))
    assert not AffineTileDopri.shapes_ok(NeuralODEModel(12, 10))
    assert not AffineTileDopri.shapes_ok(NeuralODEModel(3, 3, 6, hidden_dim=256))


def test_entry_points_are_declared():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    for name in ("nlbac_node_dopri_tile_ok", "nlbac_node_dopri_tile_fwd", "nlbac_node_dopri_tile_bwd"):
        assert name in _lib.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in header
