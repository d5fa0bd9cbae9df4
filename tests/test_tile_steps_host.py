"""Host-side checks of ``tile_steps=`` on ``rollout`` and ``odeint_dense`` (no GPU needed): every refusal comes before
anything touches a device — with every device entry patched to fail, ``test_odeint_dense_tile_host``'s ``no_device`` —
``tile_steps=None`` is the call as it was, the four ``*_paged_*`` entry points are declared in the header and in
``_lib``, and they refuse bad arguments with a message before anything is launched."""
import os
import re

import pytest
import torch

from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)
from test_odeint_dense_tile_host import GRID, model, no_device, y0_of      # noqa: F401
from test_rollout_tile_host import args, tile_args

PAGED = {"nlbac_node_dopri_tile_paged_fwd": "nlbac_node_dopri_tile_fwd",
         "nlbac_node_dopri_tile_paged_bwd": "nlbac_node_dopri_tile_bwd",
         "nlbac_node_dopri_tile_dense_paged_fwd": "nlbac_node_dopri_tile_dense_fwd",
         "nlbac_node_dopri_tile_dense_paged_bwd": "nlbac_node_dopri_tile_dense_bwd"}
H = 5


def calls(m, B=40):
    """The two entries with ``B`` rows (two tiles at 40), ``step_control="tile"`` and whatever else is given; the least
    count a tile may have in each."""
    from nlbac_amd.ode_dense import odeint_dense
    from nlbac_amd.rollout import rollout
    return ((lambda **kw: rollout(m, *args(m, B=B, H=H), method="dopri5", step_control="tile", **kw), H),
            (lambda **kw: odeint_dense(m, y0_of(m, B), GRID, step_control="tile", **kw), 1))


def test_tile_steps_goes_with_tile_only(no_device):
    from nlbac_amd.ode_dense import odeint_dense
    from nlbac_amd.rollout import rollout
    m = model()
    for kw in ({}, dict(step_control="batch")):
        for ts in ([8], "count", torch.tensor([8])):
            with pytest.raises(ValueError, match="step_control='tile'"):
                rollout(m, *args(m), method="dopri5", tile_steps=ts, **kw)
            with pytest.raises(ValueError, match="step_control='tile'"):
                odeint_dense(m, y0_of(m), GRID, tile_steps=ts, **kw)


def test_tile_steps_excludes_max_steps(no_device):
    m = model()
    for call, least in calls(m):
        for ts in ([8, 8], "count"):
            with pytest.raises(ValueError, match="max_steps"):
                call(tile_steps=ts, max_steps=8)


def test_one_entry_per_tile(no_device):
    m = model()
    for call, least in calls(m):                      # 40 rows: two tiles
        for ts in ([8], [8, 8, 8], [], torch.tensor([8, 8, 8])):
            with pytest.raises(ValueError, match="one entry per 32-row tile, 2 for 40 rows"):
                call(tile_steps=ts)
    for call, least in calls(m, B=64):                # a full last tile adds none
        with pytest.raises(ValueError, match="one entry per 32-row tile, 2 for 64 rows"):
            call(tile_steps=[8, 8, 8])


def test_entries_are_ints_of_at_least_the_least(no_device):
    m = model()
    for call, least in calls(m):
        for bad in (least - 1, 0, -3):
            with pytest.raises(ValueError, match=">= %d" % least):
                call(tile_steps=[8, bad])
            with pytest.raises(ValueError, match=">= %d" % least):
                call(tile_steps=torch.tensor([bad, 8]))
        for bad in (True, 8.0, "8", None, torch.tensor(8)):
            with pytest.raises(ValueError, match="tile_steps"):
                call(tile_steps=[8, bad])
        for bad in (torch.tensor([8.0, 8.0]), torch.tensor([True, True]), torch.tensor([[8, 8]]), torch.tensor(8)):
            with pytest.raises(ValueError, match="1-D and of an integer dtype"):
                call(tile_steps=bad)


def test_anything_else_is_refused(no_device):
    m = model()
    for call, least in calls(m):
        for bad in ("exact", "", "Count", 8, 8.0, True, object()):
            with pytest.raises(ValueError, match="tile_steps"):
                call(tile_steps=bad)


def test_a_cuda_tensor_is_asked_to_come_to_the_host(no_device, monkeypatch):
    """(No device here: the check reads the tensor's device and nothing else, so a CPU tensor that says "cuda" does.)"""
    from nlbac_amd import ode_traj

    class OnDevice(torch.Tensor):
        device = torch.device("cuda", 0)

    ts = torch.tensor([8, 8]).as_subclass(OnDevice)
    assert isinstance(ts, torch.Tensor) and ts.device.type == "cuda"
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        ode_traj.check_tile_steps("rollout", ts, 40, 1, "")
    m = model()
    for call, least in calls(m):
        with pytest.raises(ValueError, match=r"\.cpu\(\)"):
            call(tile_steps=ts)


def test_pages_times_stages_times_rows_stays_below_2_31(no_device):
    m = model()
    most = (2 ** 31 - 1) // (7 * 32)
    for call, least in calls(m):
        with pytest.raises(ValueError, match="2\\^31"):
            call(tile_steps=[most, 8])
        with pytest.raises(ValueError, match="2\\^31"):
            call(tile_steps=[most - 7, 8])
        with pytest.raises(ValueError, match="CUDA"):       # (the largest that passes gets as far as the device check)
            call(tile_steps=[most - 8, 8])


def test_good_counts_get_as_far_as_the_device_check(no_device):
    import numpy as np
    m = model()
    for call, least in calls(m):
        for ts in ([8, 9], (8, 9), torch.tensor([8, 9]), torch.tensor([8, 9], dtype=torch.int32), [np.int64(8), 9],
                   [least, least], "count"):
            with pytest.raises(ValueError, match="CUDA"):
                call(tile_steps=ts, info={})


def test_the_other_tile_checks_still_hold(no_device):
    from nlbac_amd.rollout import rollout
    m = model()
    with pytest.raises(ValueError, match="fixed grid"):
        rollout(m, *args(m), method="rk4", step_control="tile", tile_steps=[8])
    with pytest.raises(NotImplementedError, match="adjoint"):
        rollout(m, *args(m), method="dopri5", step_control="tile", tile_steps=[8], adjoint=True)
    for call, least in calls(model("concat")):
        with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
            call(tile_steps=[8, 8])
    for call, least in calls(model(hidden_dim=256)):
        with pytest.raises(NotImplementedError, match="nlbac_node_dopri_tile_ok"):
            call(tile_steps="count")
    for call, least in calls(m):
        with pytest.raises(ValueError, match="info"):
            call(tile_steps=[8, 8], info=[])


class Reached(Exception):
    pass


def test_none_is_the_rollout_as_it_was(monkeypatch):
    """``tile_steps=None`` hands ``ode_traj.solve`` what a call that never mentions it hands it: ``TileSteps`` with the
    same ``max_steps`` and ``info`` — the attributes ``test_rollout_tile_host`` sees — and no per-tile counts."""
    from nlbac_amd import ode_traj, rollout as R
    m = model()
    seen = []

    def solve(func, iv, method, mode, one_launch, x0, u, xs, *tol):
        seen.append((type(iv), dict(vars(iv)), method, mode, one_launch, tol))
        raise Reached

    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_check_device", lambda x0, controls: None)
    info = {}
    for max_steps, want in ((None, 8 * H), (7, 7)):
        del seen[:]
        for kw in ({}, dict(tile_steps=None)):
            with pytest.raises(Reached):
                R.rollout(m, *args(m, H=H), method="dopri5", step_control="tile", max_steps=max_steps, info=info, **kw)
        a, b = seen
        assert a == b and a[0] is ode_traj.TileSteps
        assert (a[1]["max_steps"], a[1]["info"] is info, a[1]["tile_steps"], a[2], a[4]) == (want, True, None, "dopri5", True)
    # the batch-wide control with tile_steps=None: EqualSteps with nothing added
    del seen[:]
    for kw in ({}, dict(tile_steps=None)):
        with pytest.raises(Reached):
            R.rollout(m, *args(m, H=H), method="dopri5", **kw)
    assert seen[0] == seen[1] and seen[0][0] is ode_traj.EqualSteps and set(seen[0][1]) == {"dt", "H"}


def test_counts_reach_the_rollout_solve_as_an_int32_tensor(monkeypatch):
    from nlbac_amd import ode_traj, rollout as R
    m = model()
    seen = {}

    def solve(func, iv, method, mode, one_launch, x0, u, xs, *tol):
        seen.update(iv=iv, one=one_launch)
        raise Reached

    monkeypatch.setattr(ode_traj, "solve", solve)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    monkeypatch.setattr(R, "_check_device", lambda x0, controls: None)
    for ts, want in (([8, 9], (8, 9)), (torch.tensor([5, 6], dtype=torch.int32), (5, 6)), ("count", "count")):
        with pytest.raises(Reached):
            R.rollout(m, *args(m, B=40, H=H), method="dopri5", step_control="tile", tile_steps=ts)
        iv = seen["iv"]
        assert type(iv) is ode_traj.TileSteps and iv.max_steps is None and seen["one"]
        if want == "count":
            assert iv.tile_steps == "count"
        else:
            assert (iv.tile_steps.dtype, iv.tile_steps.tolist()) == (torch.int32, list(want))


def test_none_is_the_dense_solve_as_it_was(monkeypatch):
    from nlbac_amd import ode_dense as OD
    m = model()
    seen = []

    def apply(*a):
        seen.append(a)
        raise Reached

    monkeypatch.setattr(OD.SolveNode, "apply", staticmethod(apply))
    monkeypatch.setattr(OD, "_check_device", lambda y0: None)
    monkeypatch.setattr(type(m), "refresh_device_weights", lambda self: None)
    y0 = y0_of(m, 40)
    for max_steps, want in ((None, 32), (7, 7)):
        for kw in ({}, dict(tile_steps=None)):
            with pytest.raises(Reached):
                OD.odeint_dense(m, y0, GRID, step_control="tile", max_steps=max_steps, **kw)
            solve = seen[-1][0]
            assert type(solve) is OD._DenseTileSolve and solve.slots == want and solve.tile_steps is None
    for ts, want in (([8, 9], (8, 9)), (torch.tensor([5, 6]), (5, 6)), ("count", "count")):
        with pytest.raises(Reached):
            OD.odeint_dense(m, y0, GRID, step_control="tile", tile_steps=ts)
        solve = seen[-1][0]
        assert type(solve) is OD._DenseTileSolve and solve.slots is None
        if want == "count":
            assert solve.tile_steps == "count"
        else:
            assert (solve.tile_steps.dtype, solve.tile_steps.tolist()) == (torch.int32, list(want))


def test_entry_points_are_declared():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in raw
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, sibling in PAGED.items():
        assert name in _lib.EXPORTS
        proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name]) == len(_lib._PROTOS[sibling]) + 1, name
        assert "const int *page0, int pages" in proto and "max_slots" not in proto, name
        # the sibling's arguments with (page0, pages) in place of max_slots, in the header and in _lib
        sib = re.search(r"int %s\s*\((.*?)\);" % sibling, txt, flags=re.S).group(1)
        flat = lambda s: re.sub(r"\s+", " ", s)
        assert flat(proto) == flat(sib).replace("int max_slots", "const int *page0, int pages"), name
        k = [a.strip() for a in flat(sib).split(",")].index("int max_slots")
        want = list(_lib._PROTOS[sibling])
        want[k:k + 1] = [_lib._P, _lib._I]
        assert list(_lib._PROTOS[name]) == want, name


def paged_args(lib, name):
    """``tile_args`` of the sibling with (page0, pages) in place of max_slots: 8 rows are one tile with two pages."""
    kw, keep = tile_args(lib, PAGED[name])
    out = {}
    for k, v in kw.items():
        if k == "max_slots":
            out["page0"], out["pages"] = kw["hslots"], v
        else:
            out[k] = v
    from nlbac_amd import _lib
    assert len(out) == len(_lib._PROTOS[name]), name
    return out, keep


@pytest.mark.parametrize("name", sorted(PAGED))
def test_paged_entries_refuse_before_launching(lib, name):
    kw, keep = paged_args(lib, name)
    fwd, dense = name.endswith("_fwd"), "_dense_" in name
    assert "page0" in refused(lib, name, dict(kw, page0=None), "a null page0 with pages > 0")
    assert "2^31" in refused(lib, name, dict(kw, pages=2 ** 31 // (7 * 32) + 1), "the least pages * 7 * 32 >= 2^31")
    assert "2^31" in refused(lib, name, dict(kw, pages=2 ** 31 - 1), "pages * 7 * 32 far beyond 2^31")
    if fwd:
        assert "go together" in refused(lib, name, dict(kw, hslots=None), "kept steps without hslots")
        assert "page0" in refused(lib, name, dict(kw, pages=0), "page0 with no pages")
    else:
        assert "null pointer" in refused(lib, name, dict(kw, hslots=None), "a null hslots")
    # a page per interval and tile at least (H = 2 in the rollout's arguments; 1 for the dense solve)
    if not dense:
        assert "pages must be at least H" in refused(lib, name, dict(kw, pages=1), "fewer pages than intervals")
    # the siblings' refusals come through the same fill
    assert "null pointer" in refused(lib, name, dict(kw, f=None), "a null f")
    assert "acts_bits is 0, 1 or 2" in refused(lib, name, dict(kw, bits=3), "acts_bits = 3")
    assert "bad rows" in refused(lib, name, dict(kw, n=0), "n = 0")
