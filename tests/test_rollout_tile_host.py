"""Host-side checks of ``rollout(..., step_control=, max_steps=, info=)``: every refusal comes before anything touches a
device (CPU tensors reach it), ``step_control="batch"`` is the call as it was, the three
``nlbac_node_dopri_tile_*`` entry points are declared, and ``nlbac_node_dopri_tile_{fwd,bwd}`` refuse bad arguments with
a message before anything is launched (no GPU needed: every pointer handed over there is host memory that a refused call
never touches)."""
import ctypes as C
import os
import re

import pytest
import torch

from test_rollout_concat_host import desc, lib, refused      # noqa: F401  (lib: the fixture that builds and loads)


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


def test_tableau_serves_dopri5():
    """``_tableau("dopri5")``: the table's rows give the stage count, row i of DP_BETA is row i + 1 of the flat table,
    and a method without solution weights has no ``c_out``."""
    from nlbac_amd.ode_consts import DP_BETA
    from nlbac_amd.ode_traj import _tableau
    S, beta, c_out = _tableau("dopri5")
    assert S == 7 and len(beta) == 49 and c_out is None
    want = [0.0] * 49
    for i, row in enumerate(DP_BETA):
        for j, v in enumerate(row):
            want[(i + 1) * 7 + j] = C.c_float(v).value
    assert list(beta) == want


def tile_args(lib, name):
    """The arguments of a call of the tile entry point ``name`` that would be launched — a solve of 8 rows that keeps
    activation rows in 2 slots per tile (forward), its backward from mask words without weight gradients — by name and
    in the entry point's order."""
    from nlbac_amd import _lib
    dense, fwd = "_dense_" in name, name.endswith("_fwd")
    host = (C.c_float * 64)()                    # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    nets = (desc(lib, 5, 3, 64, 3), desc(lib, 4, 3, 64, 6))
    assert lib.nlbac_node_dopri_tile_ok(C.byref(nets[0]), C.byref(nets[1])) == 1
    head = dict(f=C.byref(nets[0]), g=C.byref(nets[1]))
    beta, c_err = _lib.fptr(*([0.0] * 49)), _lib.fptr(*([0.0] * 7))
    rows, words = 2 * 7 * 8 * 64, 2 * 7 * 8 * 4
    if fwd:
        solve = (dict(n=8, beta=beta, c_err=c_err, tau=p, n_out=2, t_end=0.02) if dense else
                 dict(n=8, H=2, beta=beta, c_err=c_err, dt=0.02))
        slots = dict(hslots=p, ov_slot=p, ov_x=p) if dense else dict(hslots=p, iv_first=p, iv_x=p)
        kw = dict(head, x0=p, u=p, **solve, rtol=1e-5, atol=1e-7, out=p, max_slots=2, Y=p, G=p, acts_f=p, ls_f=rows,
                  acts_g=p, ls_g=rows, bits=0, **slots, accepted=p, attempts=p, status=p, s=None)
    else:
        solve = (dict(n=8, beta=beta, n_out=2, max_slots=2, hslots=p, ov_slot=p, ov_x=p, nacc=p) if dense else
                 dict(n=8, H=2, beta=beta, max_slots=2, hslots=p, iv_first=p, iv_nacc=p, iv_x=p))
        kw = dict(head, u=p, **solve, G=p, acts_f=p, ls_f=words, acts_g=p, ls_g=words, bits=1, dout=p, dx0=p, du=p,
                  dK=None, dG=None, dz_f=None, dz_g=None, s=None)
    assert len(kw) == len(_lib._PROTOS[name]), name
    return kw, (nets, host, beta, c_err)


def forward_refusals(lib, name):
    """What both tile forwards refuse, one changed argument each."""
    kw, keep = tile_args(lib, name)
    wide = (desc(lib, 5, 3, 256, 3), desc(lib, 4, 3, 256, 6))
    length = "t_end" if "_dense_" in name else "dt"
    assert "null pointer" in refused(lib, name, dict(kw, f=None), "a null f")
    assert "nlbac_node_dopri_tile_ok" in refused(lib, name, dict(kw, f=C.byref(wide[0]), g=C.byref(wide[1])), "256-wide nets")
    assert "bad rows" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "acts_bits is 0, 1 or 2" in refused(lib, name, dict(kw, bits=3), "acts_bits = 3")
    assert "null pointer" in refused(lib, name, dict(kw, x0=None), "a null x0")
    assert "bad interval / tolerances" in refused(lib, name, dict(kw, **{length: 0.0}), "an interval of 0")
    assert "bad interval / tolerances" in refused(lib, name, dict(kw, rtol=0.0, atol=0.0), "rtol = atol = 0")
    assert "go together" in refused(lib, name, dict(kw, acts_g=None), "acts_f without acts_g")
    together = "G, the acts and the slot arrays go together"
    assert together in refused(lib, name, dict(kw, hslots=None), "G without hslots")
    assert together in refused(lib, name, dict(kw, G=None), "Y without G")


def backward_refusals(lib, name):
    """What both tile backwards refuse, one changed argument each."""
    kw, keep = tile_args(lib, name)
    p = kw["dout"]
    assert "null pointer" in refused(lib, name, dict(kw, dout=None), "a null dout")
    assert "dz_f, dz_g, dG and dK go together" in refused(lib, name, dict(kw, dz_f=p, dz_g=p, dG=p), "dz_f without dK")
    assert "weight gradients need the activations" in refused(lib, name, dict(kw, dK=p, dG=p, dz_f=p, dz_g=p),
                                                              "acts_bits = 1 with the weight-gradient rows")


def test_forward_refuses_before_launching(lib):
    name = "nlbac_node_dopri_tile_fwd"
    forward_refusals(lib, name)
    kw, keep = tile_args(lib, name)
    assert "bad rows / intervals" in refused(lib, name, dict(kw, H=0), "H = 0")
    assert "max_slots must be at least H" in refused(lib, name, dict(kw, max_slots=1), "fewer slots than intervals")


def test_backward_refuses_before_launching(lib):
    name = "nlbac_node_dopri_tile_bwd"
    backward_refusals(lib, name)
    kw, keep = tile_args(lib, name)
    assert "max_slots must be at least H" in refused(lib, name, dict(kw, max_slots=1), "fewer slots than intervals")
