"""GPU: ``rollout(method="dopri5", step_control="tile")`` — every 32-row tile an adaptive solve of its own, the whole
horizon in one launch — against its definition: the rows of tile j are today's chained ``rollout(method="dopri5")`` on
those rows alone, values and gradients.  Nothing else is the reference.

The inputs make the tiles differ: ``x0`` and ``controls`` are scaled per tile by (0.05, 1, 20) and dt = 0.5, so that more
than one step is kept per interval and (Pvtol) attempts are rejected; the first test pins that on the CPU oracle.

Seen on the MI355X: every comparison of states and input gradients holds by ``torch.equal``; the largest relative
parameter-gradient difference (norm, per tensor) against the float64 sum of the slices' gradients is 1.15e-7 (Unicycle)
and 1.08e-7 (Pvtol) — ``test_parameter_gradients`` prints every figure before it asserts."""
import pytest
import torch

from oracle import nlbac_oracle as O
from test_rollout_gpu import inputs, make

pytestmark = pytest.mark.gpu

B, H, DT = 80, 3, 0.5
SCALE = (0.05, 1.0, 20.0)
KINDS = ["unicycle", "pvtol"]
# accepted (rejected) attempts per interval of the slices' solves, from the CPU oracle (as one CPU gives them)
EXPECT = {"unicycle": [[(3, 0)] * 3, [(3, 0)] * 3, [(5, 0), (6, 0), (6, 0)]],
          "pvtol": [[(3, 0)] * 3, [(3, 0)] * 3, [(6, 1), (7, 2), (6, 0)]]}


def tiles(n):
    return [(lo, min(lo + 32, n)) for lo in range(0, n, 32)]


def scaled(kind):
    m, ns, nc = make(kind)
    x0, c = inputs(ns, nc, B, H, seed=3)
    for (lo, hi), s in zip(tiles(B), SCALE):
        x0[lo:hi] *= s
        c[:, lo:hi] *= s
    w = torch.randn(H + 1, B, ns, generator=torch.Generator().manual_seed(5))
    return m, ns, nc, x0, c, w


def run(m, x0, c, w, dt, mode, **kw):
    """One rollout in keep mode ``mode`` ("none", "inputs", "params"): out, d/dx0, d/dcontrols, the parameters' gradients."""
    from nlbac_amd.rollout import rollout
    for p in m.parameters():
        p.requires_grad_(mode == "params")
        p.grad = None
    if mode == "none":
        with torch.no_grad():
            return rollout(m, x0.cuda(), c.cuda(), dt, method="dopri5", **kw), None, None, []
    x0d, cd = x0.cuda().requires_grad_(), c.cuda().requires_grad_()
    out = rollout(m, x0d, cd, dt, method="dopri5", **kw)
    (out * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x0d.grad, cd.grad, [p.grad.clone() for p in m.parameters()] if mode == "params" else []


_REF = {}


def reference(kind, mode):
    """Today's chained rollout on every tile's slice, once per (model, keep mode); shared, never modified."""
    if (kind, mode) not in _REF:
        m, ns, nc, x0, c, w = scaled(kind)
        _REF[(kind, mode)] = [run(m, x0[lo:hi], c[:, lo:hi], w[:, lo:hi], DT, mode) for lo, hi in tiles(B)]
    return _REF[(kind, mode)]


@pytest.mark.parametrize("kind", KINDS)
def test_input_conditions_on_the_oracle(kind):
    m, ns, nc, x0, c, w = scaled(kind)
    ref = O.AffineNode({k: v.detach().clone() for k, v in m.state_dict().items()}, n_s=ns, n_u=nc)
    t = torch.tensor([0.0, DT])
    for j, (lo, hi) in enumerate(tiles(B)):
        x, got = x0[lo:hi], []
        with torch.no_grad():
            for k in range(H):
                info = {}
                x = O.odeint(ref, torch.cat([x, c[k, lo:hi]], 1), t, method="dopri5", info=info)[-1][:, :ns]
                acc = sum(1 for s in info["steps"] if s[2])
                got.append((acc, len(info["steps"]) - acc))
        print(kind, "tile", j, got)
        # the accepted steps (the slots a backward keeps) are the table's; an attempt whose error ratio sits at the
        # accept threshold falls either way with the host's float32 kernels (interval 0 of Pvtol's tile 2: one rejection
        # on one CPU, two on another), so of the rejected ones only "none" / "some" is pinned
        assert [a for a, _ in got] == [a for a, _ in EXPECT[kind][j]], (kind, j, got)
        assert [r > 0 for _, r in got] == [r > 0 for _, r in EXPECT[kind][j]], (kind, j, got)


@pytest.mark.parametrize("kind", KINDS)
def test_values(kind):
    m, ns, nc, x0, c, w = scaled(kind)
    info = {}
    out = run(m, x0, c, w, DT, "none", step_control="tile", info=info)[0]
    ref = reference(kind, "none")
    assert out.shape == (H + 1, B, ns)
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(out[:, lo:hi], ref[j][0]), "tile %d" % j
    acc, att, status = info["accepted"].cpu(), info["attempts"].cpu(), info["status"].cpu()
    print(kind, "accepted", acc.tolist(), "attempts", att.tolist())
    assert acc.shape == (3, H) and att.shape == (3, H) and acc.dtype == torch.int32
    assert status.tolist() == [0, 0, 0]
    assert bool((acc[2] > acc[0]).all())
    assert bool((att >= acc).all())
    if kind == "pvtol":
        assert bool((att > acc).any())


@pytest.mark.parametrize("kind", KINDS)
def test_input_gradients(kind):
    m, ns, nc, x0, c, w = scaled(kind)
    out, dx, dc, _ = run(m, x0, c, w, DT, "inputs", step_control="tile", max_steps=32)
    ref = reference(kind, "inputs")
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(out[:, lo:hi], ref[j][0]), "out, tile %d" % j
        assert torch.equal(dx[lo:hi], ref[j][1]), "d/dx0, tile %d" % j
        assert torch.equal(dc[:, lo:hi], ref[j][2]), "d/dcontrols, tile %d" % j


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_gradients(kind):
    m, ns, nc, x0, c, w = scaled(kind)
    out, dx, dc, gp = run(m, x0, c, w, DT, "params", step_control="tile", max_steps=32)
    ref = reference(kind, "params")
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(out[:, lo:hi], ref[j][0]), "out, tile %d" % j
        assert torch.equal(dx[lo:hi], ref[j][1]), "d/dx0, tile %d" % j
        assert torch.equal(dc[:, lo:hi], ref[j][2]), "d/dcontrols, tile %d" % j
    errs = []
    for i, a in enumerate(gp):
        b = sum(r[3][i].double() for r in ref)
        errs.append(float((a.double() - b).norm()) / max(1e-12, float(b.norm())))
    print(kind, "parameter gradients, relative difference (norm) per tensor:", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("hid", [64, 128])
def test_other_widths(hid):
    """The kernel instances of the other two widths the register-resident kernels serve (the tests above run width 100):
    values without gradients, then values and input gradients, against the slices."""
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6, hidden_dim=hid)
    _, ns, nc, x0, c, w = scaled("unicycle")
    ref = {mode: [run(m, x0[lo:hi], c[:, lo:hi], w[:, lo:hi], DT, mode) for lo, hi in tiles(B)] for mode in ("none", "inputs")}
    info = {}
    out = run(m, x0, c, w, DT, "none", step_control="tile", info=info)[0]
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(out[:, lo:hi], ref["none"][j][0]), "no gradients, tile %d" % j
    assert info["status"].tolist() == [0, 0, 0]
    out, dx, dc, _ = run(m, x0, c, w, DT, "inputs", step_control="tile", max_steps=32)
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(out[:, lo:hi], ref["inputs"][j][0]), "out, tile %d" % j
        assert torch.equal(dx[lo:hi], ref["inputs"][j][1]), "d/dx0, tile %d" % j
        assert torch.equal(dc[:, lo:hi], ref["inputs"][j][2]), "d/dcontrols, tile %d" % j


def test_many_workgroups_and_a_ragged_end():
    n, h, dt = 8208, 2, 0.02
    m, ns, nc = make("unicycle")
    x0, c = inputs(ns, nc, n, h, seed=3)
    w = torch.randn(h + 1, n, ns, generator=torch.Generator().manual_seed(5))
    info = {}
    out, dx, dc, _ = run(m, x0, c, w, dt, "inputs", step_control="tile", info=info)
    ts = tiles(n)
    assert len(ts) == 257 and ts[-1] == (8192, 8208)
    for j in (0, 128, 255, 256):
        lo, hi = ts[j]
        o, gx, gc, _ = run(m, x0[lo:hi], c[:, lo:hi], w[:, lo:hi], dt, "inputs")
        assert torch.equal(out[:, lo:hi], o), "out, tile %d" % j
        assert torch.equal(dx[lo:hi], gx), "d/dx0, tile %d" % j
        assert torch.equal(dc[:, lo:hi], gc), "d/dcontrols, tile %d" % j
    assert info["accepted"].shape == (257, h) and bool((info["accepted"] == 1).all())
    assert bool((info["status"] == 0).all())


def test_one_launch_and_no_host_look(monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_ctl import ControlBlockReader
    from nlbac_amd.rollout import rollout
    m, ns, nc, x0, c, w = scaled("pvtol")
    for p in m.parameters():
        p.requires_grad_(False)
    x0d, cd = x0.cuda().requires_grad_(), c.cuda().requires_grad_()
    calls, looks = [], []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(ControlBlockReader, "read", lambda self, *a, **k: looks.append(1))
    out = rollout(m, x0d, cd, DT, method="dopri5", step_control="tile", max_steps=32)
    # (every rollout refreshes the weight copies first, as odeint does: nlbac_mlp_pack is not part of the solve)
    assert [n for n in calls if n != "nlbac_mlp_pack"] == ["nlbac_node_dopri_tile_fwd"], calls
    del calls[:]
    (out * w.cuda()).sum().backward()
    assert calls == ["nlbac_node_dopri_tile_bwd"], calls
    assert not looks


def test_out_of_slots():
    from nlbac_amd._lib import NlbacError
    from nlbac_amd.rollout import rollout
    """Slots are counted per tile over the whole horizon: tiles 0 and 1 keep 3 + 3 + 3 = 9 steps, tile 2 would keep
    6 + 7 + 6 = 19.  With max_steps = 9 — the fewest with which tiles 0 and 1 finish, their last step in their last
    slot — tile 2 runs out in its second interval.  (max_steps = 6 stops all three tiles: 9 > 6.)"""
    m, ns, nc, x0, c, w = scaled("pvtol")
    assert [sum(a for a, _ in t) for t in EXPECT["pvtol"]] == [9, 9, 19]
    for p in m.parameters():
        p.requires_grad_(False)
    x0d, cd = x0.cuda().requires_grad_(), c.cuda().requires_grad_()
    info = {}
    out = rollout(m, x0d, cd, DT, method="dopri5", step_control="tile", max_steps=9, info=info)
    assert info["status"].tolist() == [0, 0, 1]
    assert bool(torch.isnan(out[-1, 64:80]).all()) and bool(torch.isnan(out[2, 64:80]).all())
    assert bool(torch.isfinite(out[:2, 64:80]).all())      # (6 slots taken by interval 0, the other 3 run out in interval 1)
    assert info["accepted"][2].tolist() == [6, 0, 0]
    ref = reference("pvtol", "inputs")
    for j, (lo, hi) in enumerate(tiles(B)[:2]):
        assert torch.equal(out[:, lo:hi].detach(), ref[j][0]), "tile %d" % j
    with pytest.raises(NlbacError, match="max_steps"):
        out[:, :64].sum().backward()
    info = {}
    with torch.no_grad():
        out = rollout(m, x0.cuda(), c.cuda(), DT, method="dopri5", step_control="tile", max_steps=9, info=info)
    assert info["status"].tolist() == [0, 0, 0]
    assert bool(torch.isfinite(out).all())


def test_the_default_is_untouched():
    m, ns, nc, x0, c, w = scaled("unicycle")
    a = run(m, x0, c, w, DT, "params")
    b = run(m, x0, c, w, DT, "params", step_control="batch")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) > 0
    for ga, gb in zip(a[3], b[3]):
        assert torch.equal(ga, gb)
