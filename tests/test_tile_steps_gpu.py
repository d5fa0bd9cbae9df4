"""GPU: ``tile_steps=`` on ``rollout(method="dopri5", step_control="tile")`` and ``odeint_dense(step_control="tile")`` —
the step slots counted per tile, the kept buffers in pages of 7 stages x 32 rows — against the same call with
``max_steps=32`` (which ``test_rollout_tile_gpu`` / ``test_odeint_dense_tile_gpu`` hold against the slices' solves): values
and input gradients bit for bit; the parameter gradients, whose sums run over the rows in another order by
construction, against the float64 sum of the slices' gradients at those tests' bar of 1e-5, every figure printed first.

The inputs are those two modules': 80 rows in tiles of 32 / 32 / 16, scaled so that the tiles differ.  The exact counts
are read off a ``max_steps=32`` run's ``info["accepted"]`` and held against the modules' tables: 9 / 9 / 19 (Pvtol
rollout), 9 / 9 / 17 (Unicycle rollout), 5 / 9 / 20 (dense solve)."""
import pytest
import torch

import test_odeint_dense_tile_gpu as DT
import test_rollout_tile_gpu as RT
from test_odeint_dense_gpu import node_of
from test_rollout_gpu import inputs, make

pytestmark = pytest.mark.gpu

CASES = ["unicycle", "pvtol", "dense"]
COUNTS = {"unicycle": [9, 9, 17], "pvtol": [9, 9, 19], "dense": [5, 9, 20]}
PACK = "nlbac_mlp_pack"      # (every solve refreshes the weight copies first: not part of the solve)


class Case:
    """One of the three solves: ``run(mode, **kw)`` -> (out, the input gradients, the parameter gradients) under
    ``step_control="tile"``; ``sliced(mode)``: the existing modules' references on the tiles' slices (out, input gradients,
    parameter gradients per slice); the entry points' names and where ``page0`` sits in the paged forward's arguments."""

    def __init__(self, name):
        self.name, self.dense = name, name == "dense"
        if self.dense:
            self.y0, self.t, self.dout = DT.scaled()
            self.m = node_of("unicycle")
            self.fwd, self.bwd = "nlbac_node_dopri_tile_dense_fwd", "nlbac_node_dopri_tile_dense_bwd"
            self.pfwd, self.pbwd = "nlbac_node_dopri_tile_dense_paged_fwd", "nlbac_node_dopri_tile_dense_paged_bwd"
            self.at = 13
        else:
            self.m, self.ns, self.nc, self.x0, self.c, self.w = RT.scaled(name)
            self.fwd, self.bwd = "nlbac_node_dopri_tile_fwd", "nlbac_node_dopri_tile_bwd"
            self.pfwd, self.pbwd = "nlbac_node_dopri_tile_paged_fwd", "nlbac_node_dopri_tile_paged_bwd"
            self.at = 12
        self.hid = [l for l in self.m.f_net.modules() if isinstance(l, torch.nn.Linear)][0].out_features

    def run(self, mode, **kw):
        if self.dense:
            out, gy, gp = DT.run(self.m, self.y0, self.t, self.dout, mode, step_control="tile", **kw)
            return out, (gy,), gp
        out, dx, dc, gp = RT.run(self.m, self.x0, self.c, self.w, RT.DT, mode, step_control="tile", **kw)
        return out, (dx, dc), gp

    def sliced(self, mode):
        if self.dense:
            return [(r[0], (r[1],), r[2]) for r in DT.reference(mode)]
        return [(r[0], (r[1], r[2]), r[3]) for r in RT.reference(self.name, mode)]


_CASE, _MAX32, _ACC = {}, {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = Case(name)
    return _CASE[name]


def max32(name, mode):
    """The ``max_steps=32`` call, once per (solve, keep mode); shared, never modified."""
    if (name, mode) not in _MAX32:
        info = {}
        _MAX32[(name, mode)] = case(name).run(mode, max_steps=32, info=info)
        if mode != "none":
            assert info["status"].tolist() == [0, 0, 0]
            _ACC[name] = info["accepted"].reshape(3, -1).sum(1).tolist()
    return _MAX32[(name, mode)]


def counts(name):
    """The tiles' accepted steps of the ``max_steps=32`` run — the tables' counts."""
    if name not in _ACC:
        max32(name, "inputs")
    assert _ACC[name] == COUNTS[name], (name, _ACC[name])
    return list(_ACC[name])


def same_values(got, ref, what):
    assert torch.equal(got[0], ref[0]), "%s: out" % what
    if ref[1][0] is not None:
        for i, (a, b) in enumerate(zip(got[1], ref[1])):
            assert torch.equal(a, b), "%s: input gradient %d" % (what, i)


def parameter_gradients(name, gp, what):
    ref = case(name).sliced("params")
    errs = []
    for i, a in enumerate(gp):
        b = sum(r[2][i].double() for r in ref)
        errs.append(float((a.double() - b).norm()) / max(1e-12, float(b.norm())))
    print(name, what, "parameter gradients, relative difference (norm) per tensor:", ["%.2e" % e for e in errs])
    assert len(errs) > 0 and max(errs) <= 1e-5, errs


def test_the_counts_are_the_tables():
    assert [sum(a for a, _ in t) for t in RT.EXPECT["pvtol"]] == COUNTS["pvtol"]
    assert [sum(a for a, _ in t) for t in RT.EXPECT["unicycle"]] == COUNTS["unicycle"]
    assert [e[0] for e in DT.EXPECT] == COUNTS["dense"]
    for name in CASES:
        assert counts(name) == COUNTS[name]


@pytest.mark.parametrize("mode", ["none", "inputs", "params"])
@pytest.mark.parametrize("name", CASES)
def test_exact_counts_agree_with_max_steps(name, mode):
    ts = counts(name)
    ref = max32(name, mode)
    info = {}
    got = case(name).run(mode, tile_steps=ts, info=info)
    same_values(got, ref, "%s, %s" % (name, mode))
    assert info["status"].tolist() == [0, 0, 0]
    assert info["slots"].dtype == torch.int32 and info["slots"].device.type == "cpu" and info["slots"].tolist() == ts
    assert info["accepted"].reshape(3, -1).sum(1).tolist() == ts
    if mode == "params":
        parameter_gradients(name, got[2], "exact counts")
        # a CPU tensor is the same call
        again = case(name).run(mode, tile_steps=torch.tensor(ts))
        same_values(again, ref, "%s, counts as a tensor" % name)
        for a, b in zip(again[2], got[2]):
            assert torch.equal(a, b)


def traced(monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_ctl import ControlBlockReader
    calls, looks = [], []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    monkeypatch.setattr(ControlBlockReader, "read", lambda self, *a, **k: looks.append(1))
    return calls, looks


@pytest.mark.parametrize("mode", ["inputs", "params"])
@pytest.mark.parametrize("name", CASES)
def test_kept_buffers_are_page_sized(name, mode, monkeypatch):
    """The paged forward's arguments: ``pages`` is sum(counts) and the layers' stride that many pages x 7 stages x 32
    rows (x 4 mask words, or x hid activations); one paged launch each way, + the weight-gradient launch over exactly
    those rows; nobody reads a control block."""
    from nlbac_amd import ode_traj
    k, ts = case(name), counts(name)
    pages = sum(ts)
    rows = pages * 7 * 32
    assert rows < max(ts) * 3 * 7 * 32 and rows < 32 * 7 * 80      # fewer than max * n_tiles pages, and than max_steps = 32
    kept = []
    init = ode_traj.AffineTile.__init__
    monkeypatch.setattr(ode_traj.AffineTile, "__init__", lambda self, *a, **kw: (kept.append(self), init(self, *a, **kw))[1])
    calls, looks = traced(monkeypatch)
    got = k.run(mode, tile_steps=ts)
    names = [n for n, _ in calls if n != PACK]
    want = [k.pfwd, k.pbwd] + (["nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"] if mode == "params" else [])
    assert names == want, names
    assert not looks
    fwd = dict(calls)[k.pfwd]
    page0, n_pages, Y, G, acts_f, ls_f, acts_g, ls_g = fwd[k.at:k.at + 8]
    assert page0 and G and acts_f and acts_g and n_pages == pages
    per = k.hid if mode == "params" else 4
    assert (ls_f, ls_g) == (rows * per, rows * per) and bool(Y) == (mode == "params")
    bwd = dict(calls)[k.pbwd]
    assert bwd[6] == page0 and bwd[7] == pages
    if mode == "params":
        assert dict(calls)["nlbac_mlp_bwd_weights"][3] == rows
    # the solve object: every kept array holds sum(counts) pages of 7 stages x 32 rows
    tile = kept[-1]
    assert tile.paged and tile.pages == pages and tile.page0.tolist() == [0, ts[0], ts[0] + ts[1], pages]
    assert tile.G.shape[:2] == (pages * 7, 32) and tile.hslots.shape == (pages,)
    assert tile.acts[0].numel() == ((k.hid + (4 if tile.bits == 2 else 0)) if mode == "params" else 4) * 4 * rows
    same_values(got, max32(name, mode), name)


def test_one_slot_short():
    """Pvtol's exact counts with tile 2 one slot short: 9 / 9 / 18.  Tiles 0 and 1 finish with their last step in their
    last slot; tile 2 keeps 6 + 7 steps in the intervals 0 and 1 and runs out in interval 2, at the fifth of its six."""
    from nlbac_amd._lib import NlbacError
    from nlbac_amd.rollout import rollout
    k, ts = case("pvtol"), counts("pvtol")
    assert ts == [9, 9, 19] and [a for a, _ in RT.EXPECT["pvtol"][2]] == [6, 7, 6]
    short = ts[:2] + [ts[2] - 1]
    for p in k.m.parameters():
        p.requires_grad_(False)
    x0d, cd = k.x0.cuda().requires_grad_(), k.c.cuda().requires_grad_()
    info = {}
    out = rollout(k.m, x0d, cd, RT.DT, method="dopri5", step_control="tile", tile_steps=short, info=info)
    assert info["status"].tolist() == [0, 0, 1]
    assert info["slots"].tolist() == short
    assert info["accepted"][2].tolist() == [6, 7, 0]
    ref, full = k.sliced("inputs"), max32("pvtol", "inputs")
    for j, (lo, hi) in enumerate(RT.tiles(RT.B)[:2]):
        assert torch.equal(out[:, lo:hi].detach(), ref[j][0]), "tile %d against its slice" % j
        assert torch.equal(out[:, lo:hi].detach(), full[0][:, lo:hi]), "tile %d against max_steps=32" % j
    assert bool(torch.isnan(out[3, 64:80]).all())
    assert torch.equal(out[:3, 64:80].detach(), full[0][:3, 64:80])
    with pytest.raises(NlbacError, match=r"tile_steps\[2\] = 18"):
        out[:, :64].sum().backward()
    info = {}
    out = rollout(k.m, x0d, cd, RT.DT, method="dopri5", step_control="tile", tile_steps=ts, info=info)
    assert info["status"].tolist() == [0, 0, 0]
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("mode", ["inputs", "params"])
@pytest.mark.parametrize("name", CASES)
def test_count(name, mode, monkeypatch):
    k, ts = case(name), counts(name)
    ref = max32(name, mode)
    calls, looks = traced(monkeypatch)
    info = {}
    got = k.run(mode, tile_steps="count", info=info)
    same_values(got, ref, "%s, %s" % (name, mode))
    assert info["slots"].tolist() == info["accepted"].reshape(3, -1).sum(1).tolist() == ts
    assert info["slots"].dtype == torch.int32 and info["slots"].device.type == "cpu"
    assert info["status"].tolist() == [0, 0, 0]
    fwds = [a for n, a in calls if n == k.pfwd]
    names = [n for n, _ in calls if n != PACK]
    assert names[:3] == [k.pfwd, k.pfwd, k.pbwd] and k.fwd not in names and k.bwd not in names, names
    # unkept (no page0, no pages, no G: the counting pass), then paged
    assert [bool(a[k.at]) for a in fwds] == [False, True] and [a[k.at + 1] for a in fwds] == [0, sum(ts)]
    assert [bool(a[k.at + 3]) for a in fwds] == [False, True]
    assert fwds[0][k.at + 8] == fwds[1][k.at + 8] and not looks      # (acts_bits: the same kernel instance)
    if mode == "params":
        parameter_gradients(name, got[2], "tile_steps='count'")


@pytest.mark.parametrize("name", CASES)
def test_count_under_no_grad_counts_nothing(name, monkeypatch):
    k = case(name)
    ref = max32(name, "none")
    calls, looks = traced(monkeypatch)
    info = {}
    got = k.run("none", tile_steps="count", info=info)
    assert torch.equal(got[0], ref[0])
    assert [n for n, _ in calls if n != PACK] == [k.pfwd]
    assert info["slots"] is None and info["status"].tolist() == [0, 0, 0]


def test_many_workgroups_and_a_ragged_end():
    """``test_rollout_tile_gpu``'s shape: 257 tiles, the last of 16 rows, every tile one step per interval."""
    n, h, dt = 8208, 2, 0.02
    m, ns, nc = make("unicycle")
    x0, c = inputs(ns, nc, n, h, seed=3)
    w = torch.randn(h + 1, n, ns, generator=torch.Generator().manual_seed(5))
    info = {}
    out, dx, dc, _ = RT.run(m, x0, c, w, dt, "inputs", step_control="tile", tile_steps=[2] * 257, info=info)
    ts = RT.tiles(n)
    assert len(ts) == 257 and ts[-1] == (8192, 8208)
    for j in (0, 128, 255, 256):
        lo, hi = ts[j]
        o, gx, gc, _ = RT.run(m, x0[lo:hi], c[:, lo:hi], w[:, lo:hi], dt, "inputs")
        assert torch.equal(out[:, lo:hi], o), "out, tile %d" % j
        assert torch.equal(dx[lo:hi], gx), "d/dx0, tile %d" % j
        assert torch.equal(dc[:, lo:hi], gc), "d/dcontrols, tile %d" % j
    assert bool((info["accepted"] == 1).all()) and bool((info["status"] == 0).all())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dc).all())


@pytest.mark.parametrize("name", CASES)
def test_the_default_call_is_unchanged(name, monkeypatch):
    k = case(name)
    ref = max32(name, "params")
    calls, looks = traced(monkeypatch)
    got = k.run("params", max_steps=32, tile_steps=None)
    names = [n for n, _ in calls if n != PACK]
    assert names == [k.fwd, k.bwd, "nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"], names
    same_values(got, ref, name)
    assert len(got[2]) == len(ref[2]) > 0
    for a, b in zip(got[2], ref[2]):
        assert torch.equal(a, b)
