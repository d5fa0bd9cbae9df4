"""GPU: ``odeint_dense(..., step_control="tile")`` — every 32-row tile one dense dopri5 solve of its own, the whole time
series in one launch — against its definition: the rows of tile j are today's ``odeint_dense`` (the batch-wide control)
on those rows alone, values and gradients, bit for bit.  Nothing else is the reference.

The inputs make the tiles differ: 80 rows of ``dense_common``'s Unicycle inputs (tiles of 32, 32 and 16 rows), states and
controls scaled per tile by (0.05, 1, 5), read at nine points up to 1.47 — the tiles take 5, 9 and 20 accepted steps,
tile 2 with a rejected attempt; steps without an output, a step with four, last steps that overshoot ``t[-1]``.  The
first test pins that on the CPU oracle.

No comparison falls back from bit equality: the tile runs the code of the launches it replaces, and
``dopri_interp_value`` / ``dopri_interp_grad`` are compiled without contraction in every kernel that inlines them.
``test_parameter_gradients`` prints the parameter gradients' relative differences (norm, per tensor) against the
float64 sum of the slices' gradients before it asserts them at 1e-5 — the sums over a tile's rows and over the tiles
are taken in another order than three solves' separate sums, so this one comparison is not bitwise by construction
(``test_rollout_tile_gpu.test_parameter_gradients``' bar and method).

Seen on the MI355X: every comparison of values and input gradients holds by ``torch.equal``; the device takes
[5, 9, 20] accepted steps in [5, 9, 21] attempts; the largest relative parameter-gradient difference is 3.32e-7."""
import pytest
import torch

import dense_common as D
from test_odeint_dense_gpu import node_of

pytestmark = pytest.mark.gpu

B = 80
SCALE = (0.05, 1.0, 5.0)
GRID = [0.0, 0.01, 0.02, 0.05, 0.3, 0.35, 0.4, 0.6, 1.47]
# accepted steps, whether any attempt was rejected, outputs per accepted step: the slices' solves on the CPU oracle
EXPECT = [(5, False, [2, 1, 4, 0, 1]),
          (9, False, [2, 1, 0, 3, 1, 0, 0, 0, 1]),
          (20, True, [2, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1])]


def tiles(n):
    return [(lo, min(lo + 32, n)) for lo in range(0, n, 32)]


def scaled():
    y0 = D._unicycle_inputs()[0][:B].clone()
    for (lo, hi), s in zip(tiles(B), SCALE):
        y0[lo:hi] *= s
    t = torch.tensor(GRID, dtype=torch.float32)
    dout = torch.randn(len(GRID), B, y0.shape[1], generator=torch.Generator().manual_seed(5))
    return y0, t, dout


def run(m, y0, t, dout, mode, solve=None, **kw):
    """One solve in keep mode ``mode`` ("none", "inputs", "params"): out, d/dy0, the parameters' gradients."""
    from nlbac_amd.ode_dense import odeint_dense
    solve = solve or odeint_dense
    for p in m.parameters():
        p.requires_grad_(mode == "params")
        p.grad = None
    if mode == "none":
        with torch.no_grad():
            return solve(m, y0.cuda(), t, **kw), None, []
    yy = y0.cuda().requires_grad_()
    out = solve(m, yy, t, **kw)
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), yy.grad, [p.grad.clone() for p in m.parameters()] if mode == "params" else []


_REF = {}


def reference(mode):
    """Today's ``odeint_dense`` on every tile's slice, once per keep mode; shared, never modified."""
    if mode not in _REF:
        y0, t, dout = scaled()
        m = node_of("unicycle")
        _REF[mode] = [run(m, y0[lo:hi], t, dout[:, lo:hi], mode) for lo, hi in tiles(B)]
    return _REF[mode]


def check_against(out, gy, ref, what=""):
    for j, (lo, hi) in enumerate(tiles(out.shape[1])):
        assert torch.equal(out[:, lo:hi], ref[j][0]), "%sout, tile %d" % (what, j)
        if gy is not None:
            assert torch.equal(gy[lo:hi], ref[j][1]), "%sd/dy0, tile %d" % (what, j)


def test_input_conditions_on_the_oracle():
    y0, t, _ = scaled()
    W = D.case("unicycle")["W"]
    node = D.CASES["unicycle"]["node"]({k: torch.tensor(v) for k, v in W.items()})
    times = D.times_of(t)
    for j, (lo, hi) in enumerate(tiles(B)):
        with torch.no_grad():
            _, steps, ends = D.dense_reference(node, y0[lo:hi], times)
        acc = sum(1 for s in steps if s[2])
        per = D.outputs_per_step(ends, times)
        print("tile", j, "accepted", acc, "rejected", len(steps) - acc, "outputs per step", per)
        # (of the rejected attempts only none / some is pinned: a ratio at the threshold falls either way between CPUs)
        assert acc == EXPECT[j][0] and per == EXPECT[j][2], (j, acc, per)
        assert (len(steps) > acc) == EXPECT[j][1], (j, steps)


def test_values():
    y0, t, dout = scaled()
    m = node_of("unicycle")
    info = {}
    out = run(m, y0, t, dout, "none", step_control="tile", info=info)[0]
    assert out.shape == (len(GRID), B, y0.shape[1])
    check_against(out, None, reference("none"))
    assert torch.equal(out[:, :, 3:], y0[:, 3:].cuda().expand(len(GRID), B, 2))      # the carried columns
    acc, att, status = info["accepted"].cpu(), info["attempts"].cpu(), info["status"].cpu()
    print("accepted", acc.tolist(), "attempts", att.tolist())
    assert acc.shape == (3,) and att.shape == (3,) and acc.dtype == torch.int32 and status.dtype == torch.int32
    assert acc.tolist() == [5, 9, 20]
    assert int(att[2]) > int(acc[2]) and bool((att >= acc).all())
    assert status.tolist() == [0, 0, 0]


def test_input_gradients():
    y0, t, dout = scaled()
    out, gy, _ = run(node_of("unicycle"), y0, t, dout, "inputs", step_control="tile", max_steps=32)
    check_against(out, gy, reference("inputs"))


def test_parameter_gradients():
    y0, t, dout = scaled()
    out, gy, gp = run(node_of("unicycle"), y0, t, dout, "params", step_control="tile", max_steps=32)
    ref = reference("params")
    check_against(out, gy, ref)
    errs = []
    for i, a in enumerate(gp):
        b = sum(r[2][i].double() for r in ref)
        errs.append(float((a.double() - b).norm()) / max(1e-12, float(b.norm())))
    print("parameter gradients, relative difference (norm) per tensor:", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("hid", [64, 128])
def test_other_widths(hid):
    """The kernel instances of the other two widths (the Unicycle NODE above is 100 wide): values without gradients,
    then values and input gradients, against the slices."""
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6, hidden_dim=hid)
    y0, t, dout = scaled()
    ref = {mode: [run(m, y0[lo:hi], t, dout[:, lo:hi], mode) for lo, hi in tiles(B)] for mode in ("none", "inputs")}
    info = {}
    out = run(m, y0, t, dout, "none", step_control="tile", info=info)[0]
    check_against(out, None, ref["none"], "no gradients: ")
    assert info["status"].tolist() == [0, 0, 0]
    out, gy, _ = run(m, y0, t, dout, "inputs", step_control="tile", max_steps=32)
    check_against(out, gy, ref["inputs"])


def test_many_workgroups_and_a_ragged_end():
    n, t = 8208, torch.tensor([0.0, 0.01, 0.02])
    gen = torch.Generator().manual_seed(3)
    y0 = torch.cat([torch.rand(n, 2, generator=gen) * 4 - 2, torch.rand(n, 1, generator=gen) * 6 - 3,
                    (torch.rand(n, 2, generator=gen) * 2 - 1) * torch.tensor([3.5, 12.0])], 1)
    dout = torch.randn(3, n, 5, generator=gen)
    m = node_of("unicycle")
    info = {}
    out, gy, _ = run(m, y0, t, dout, "inputs", step_control="tile", info=info)
    ts = tiles(n)
    assert len(ts) == 257 and ts[-1] == (8192, 8208)
    for j in (0, 128, 255, 256):
        lo, hi = ts[j]
        o, g, _ = run(m, y0[lo:hi], t, dout[:, lo:hi], "inputs")
        assert torch.equal(out[:, lo:hi], o), "out, tile %d" % j
        assert torch.equal(gy[lo:hi], g), "d/dy0, tile %d" % j
    assert info["accepted"].shape == (257,) and info["attempts"].shape == (257,) and info["status"].shape == (257,)
    assert bool((info["status"] == 0).all()) and bool((info["accepted"] >= 1).all())


def test_two_points_are_the_slices_odeint():
    """(The parameters take a gradient too: ``odeint``'s solver always keeps activation rows, and a solve that keeps mask
    words only sums f_net's output layer in two parts — ``rollout``'s note on input gradients alone.)"""
    from nlbac_amd.odeint import odeint
    y0, _, dout = scaled()
    t = torch.tensor([0.0, 0.6])
    m = node_of("unicycle")
    dense = lambda f, y, tt, **kw: odeint(f, y, tt, method="dopri5")
    out, gy, _ = run(m, y0, t, dout[:2], "params", step_control="tile")
    for j, (lo, hi) in enumerate(tiles(B)):
        o, g, _ = run(m, y0[lo:hi], t, dout[:2, lo:hi], "params", solve=dense)
        assert torch.equal(out[:, lo:hi], o), "out, tile %d" % j
        assert torch.equal(gy[lo:hi], g), "d/dy0, tile %d" % j
    o = run(m, y0, t, dout[:2], "none", step_control="tile")[0]
    for j, (lo, hi) in enumerate(tiles(B)):
        assert torch.equal(o[:, lo:hi], run(m, y0[lo:hi], t, dout[:2, lo:hi], "none", solve=dense)[0]), "no gradients, tile %d" % j


def test_one_launch_and_no_host_look(monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_ctl import ControlBlockReader
    from nlbac_amd.ode_dense import odeint_dense
    y0, t, dout = scaled()
    m = node_of("unicycle")
    for p in m.parameters():
        p.requires_grad_(False)
    yy = y0.cuda().requires_grad_()
    w = dout.cuda()
    calls, looks = [], []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(ControlBlockReader, "read", lambda self, *a, **k: looks.append(1))
    out = odeint_dense(m, yy, t, step_control="tile", max_steps=32)
    # (every solve refreshes the weight copies first, as odeint does: nlbac_mlp_pack is not part of the solve)
    assert [n for n in calls if n != "nlbac_mlp_pack"] == ["nlbac_node_dopri_tile_dense_fwd"], calls
    del calls[:]
    (out * w).sum().backward()
    assert calls == ["nlbac_node_dopri_tile_dense_bwd"], calls
    assert not looks


def test_out_of_slots():
    """With max_steps = 9 tiles 0 and 1 finish (5 and 9 steps, tile 1's last step in its last slot); tile 2 would keep
    20 and stops behind its ninth, having emitted the outputs 1 .. 6 (2 + 1 + 0 + 0 + 0 + 0 + 1 + 1 + 1)."""
    from nlbac_amd._lib import NlbacError
    from nlbac_amd.ode_dense import odeint_dense
    assert sum(EXPECT[2][2][:9]) == 6 and EXPECT[1][0] == 9
    y0, t, dout = scaled()
    m = node_of("unicycle")
    for p in m.parameters():
        p.requires_grad_(False)
    yy = y0.cuda().requires_grad_()
    info = {}
    out = odeint_dense(m, yy, t, step_control="tile", max_steps=9, info=info)
    assert info["status"].tolist() == [0, 0, 1]
    ref = reference("inputs")
    for j, (lo, hi) in enumerate(tiles(B)[:2]):
        assert torch.equal(out[:, lo:hi].detach(), ref[j][0]), "tile %d" % j
    assert bool(torch.isfinite(out[1:7, 64:80]).all())
    assert bool(torch.isnan(out[7, 64:80]).all()) and bool(torch.isnan(out[8, 64:80]).all())
    with pytest.raises(NlbacError, match="max_steps"):
        out[:, :64].sum().backward()
    info = {}
    with torch.no_grad():
        out = odeint_dense(m, y0.cuda(), t, step_control="tile", max_steps=9, info=info)
    assert info["status"].tolist() == [0, 0, 0]
    assert bool(torch.isfinite(out).all())


def test_the_default_is_untouched():
    y0, t, dout = scaled()
    m = node_of("unicycle")
    a = run(m, y0, t, dout, "params")
    b = run(m, y0, t, dout, "params", step_control="batch")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == len(b[2]) > 0
    for ga, gb in zip(a[2], b[2]):
        assert torch.equal(ga, gb)
