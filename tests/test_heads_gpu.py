"""The update's loss heads on the device, held to the float64 references and bars of ``heads_common`` (``K`` fixed on the
CPU, see there): A. the per-row entry points of ``csrc/agent_kernels.hip``, each launched on its own through the C ABI;
B. the same arithmetic fused into the MLP launches (``csrc/dy_heads.h``) — ``nlbac_mlp_fwd_gauss`` and
``nlbac_mlp_bwd_data_head`` kinds 1, 2, 3 — once per kernel family (LDS-tiled, half-panel, quarter-panel), where the row
outputs must also equal the per-row entry point's bit for bit and dz / dx those of ``nlbac_mlp_bwd_data`` fed the head's
row output.  What is one IEEE operation or a constant is held to exact equality.  Every output has a guard row and NaN
prefill, leading dimensions are wider than the logical width, ticket words are left zero, and each check prints its
device / bar ratio before it asserts."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import heads_common as H
from common import vec_close
from test_task_kernels_gpu import dev, lib, out_buf, ptr, read, stream

pytestmark = pytest.mark.gpu
NAN = float("nan")
I32 = torch.int32


def compare(op, fn, inputs, got, what, noise=None):
    """Every tensor of ``got`` against the float64 reference of ``fn`` at ``inputs``: the bar, and vec_close 1e-4 where the
    float32 reference is itself tight."""
    ref, bar = H.reference_and_bar_noisy(op, fn, inputs, noise)
    ratios = {k: H.bar_ratio(x.numpy(), ref[k], bar[k]) for k, x in got.items()}
    for k, r in ratios.items():
        print("device / bar  %-14s %-12s %-34s %.3f" % (op, k, what, r))
    for k, r in ratios.items():
        assert r <= 1.0, "%s %s (%s): %.3f of the bar (K = %d)" % (op, k, what, r, H.K[op])
        if H.f32_is_tight(fn, inputs, ref, k):
            vec_close(got[k].numpy(), ref[k].numpy(), 1e-4, "%s %s (%s)" % (op, k, what))
    return ref, bar


def sums_close(op, name, got, ref, bar, what):
    """Partial sums against float64 sums of the reference's rows, the bar summed over the same rows."""
    r = H.bar_ratio(got.numpy(), ref, bar)
    print("device / bar  %-14s %-12s %-34s %.3f" % (op, name, what, r))
    assert r <= 1.0, "%s %s (%s): %.3f of the summed bar" % (op, name, what, r)


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), "%s: not bit for bit (%d elements differ)" % (what, int((bits(a) != bits(b)).sum()))


def tickets(n):
    return torch.zeros(n, dtype=I32, device="cuda")


def wide(t, extra, g):
    """(n, w) -> device (n, w + extra), the extra columns random; returns (tensor, ld)."""
    buf = torch.randn(t.shape[0], t.shape[1] + extra, generator=g)
    buf[:, :t.shape[1]] = t
    return dev(buf), t.shape[1] + extra


# ---------------------------------------------------------------------------
# A. the per-row entry points
# ---------------------------------------------------------------------------
def launch_gauss_fwd(d_heads, heads_ld, d_eps, d_scale, d_bias, n_u, n):
    action, logp = out_buf(n, n_u + 2), out_buf(n)
    lib().call("nlbac_gauss_sample_fwd", d_heads.data_ptr(), heads_ld, d_eps.data_ptr(), d_scale.data_ptr(),
               d_bias.data_ptr(), n_u, n, action.data_ptr(), n_u + 2, logp.data_ptr(), stream())
    torch.cuda.synchronize()
    return read(action, n, n_u, "action"), read(logp, n, 1, "logp")[:, 0]


def check_gauss_fwd(t, n_u, action, logp, what):
    compare("gauss_fwd", lambda q: H.gauss_fwd(q, n_u), t, dict(action=action, logp=logp), what, H.gauss_noise(t))
    assert bool(torch.isfinite(logp).all()), "logp is not finite everywhere"
    # tanhf is exactly +-1 far out: the action is then one rounding of +-scale + bias
    x = H.gauss_x(t, n_u)
    far = x.abs() > 12
    want = (torch.sign(x).float() * t["scale"] + t["bias"])
    assert torch.equal(action[far], want[far]), "%s: action beyond |x| = 12" % what
    return int(far.sum())


@pytest.mark.parametrize("B", H.ROWS)
@pytest.mark.parametrize("n_u", [1, 2, 3, 4])
def test_gauss_sample_forward(B, n_u):
    t, _ = H.gauss_case(B, n_u)
    g = H.gen(100 + B)
    d_heads, ld = wide(t["heads"], 3, g)
    action, logp = launch_gauss_fwd(d_heads, ld, dev(t["eps"]), dev(t["scale"]), dev(t["bias"]), n_u, B)
    far = check_gauss_fwd(t, n_u, action, logp, "B%d nu%d" % (B, n_u))
    assert far > 0 or B == 1


def launch_gauss_bwd(d, t, n_u, n, rows_per_problem, mul):
    """``nlbac_gauss_sample_bwd`` on the device tensors ``d`` (heads with its ld, the sources with theirs)."""
    dheads = out_buf(n, 2 * n_u + 1)
    da = [(d["da%d" % k].data_ptr(), t["da%d" % k].shape[1]) if "da%d" % k in t else (None, 0) for k in range(3)]
    lib().call("nlbac_gauss_sample_bwd", d["heads"].data_ptr(), d["heads_ld"], d["eps"].data_ptr(), d["scale"].data_ptr(),
               n_u, n, rows_per_problem, da[0][0], da[0][1], da[1][0], da[1][1], da[2][0], da[2][1], d["alpha"].data_ptr(),
               mul, dheads.data_ptr(), 2 * n_u + 1, stream())
    torch.cuda.synchronize()
    return read(dheads, n, 2 * n_u, "dheads")


def gauss_bwd_device(t, n_u, seed):
    d = {k: dev(v) for k, v in t.items() if k != "heads"}
    d["heads"], d["heads_ld"] = wide(t["heads"], 2, H.gen(seed))
    return d


def check_gauss_bwd(fn, t, noise, n_u, dheads, what):
    compare("gauss_bwd", fn, t, dict(dheads=dheads), what, noise)
    raw, dls = t["heads"][:, n_u:], dheads[:, n_u:]
    assert bool((dls[~H.inside_of(t["heads"], n_u)] == 0).all()), "%s: d log_std outside the clamp range" % what
    edge = (raw == H.LOG_SIG_MIN) | (raw == H.LOG_SIG_MAX)
    assert bool((dls[edge] != 0).all()), "%s: d log_std on the clamp's boundaries" % what
    return int(edge.sum())


@pytest.mark.parametrize("B", H.ROWS)
@pytest.mark.parametrize("n_u,n_src,P,norm_mul", H.GAUSS_BWD_VARIANTS)
def test_gauss_sample_backward(B, n_u, n_src, P, norm_mul):
    fn, t, noise, B_norm, mul = H.gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
    dheads = launch_gauss_bwd(gauss_bwd_device(t, n_u, 110 + B), t, n_u, P * B, B, mul)
    edge = check_gauss_bwd(fn, t, noise, n_u, dheads, "B%d nu%d src%d P%d norm%d" % (B, n_u, n_src, P, norm_mul))
    assert edge > 0 or B == 1


def td_device(B):
    t = H.td_case(B)
    d = {k: dev(v) for k, v in t.items()}
    col = lambda c: d["rcm"].data_ptr() + 4 * c
    d.update(reward=col(H.RCM_COLS["reward"]), constraint=col(H.RCM_COLS["constraint"]), mask=col(H.RCM_COLS["mask"]),
             xsig=col(H.XSIG_COL))
    return t, d


def launch_td_targets(d, B, B_norm, with_next, ticket=None, mul=0.0, out=None):
    o = dict(dq=[out_buf(B) for _ in range(3)], next_q=out_buf(B) if with_next else None,
             next_l=out_buf(B) if with_next else None, partials=out_buf((B + 255) // 256, 3))
    lib().call("nlbac_td_targets", d["q1t"].data_ptr(), d["q2t"].data_ptr(), d["lt"].data_ptr(), d["nlogp"].data_ptr(),
               d["reward"], d["constraint"], d["mask"], H.RCM_LD, d["q1"].data_ptr(), d["q2"].data_ptr(), d["lf"].data_ptr(),
               d["alpha"].data_ptr(), H.GAMMA, B, B_norm, *[b.data_ptr() for b in o["dq"]], ptr(o["next_q"]), ptr(o["next_l"]),
               o["partials"].data_ptr(), ptr(ticket), mul, ptr(out), stream())
    torch.cuda.synchronize()
    got = dict(dq=torch.cat([read(b, B, 1, "dq") for b in o["dq"]], 1))
    if with_next:
        got.update(next_q=read(o["next_q"], B, 1, "next_q")[:, 0], next_l=read(o["next_l"], B, 1, "next_l")[:, 0])
    return got, read(o["partials"], (B + 255) // 256, 3, "partials")


@pytest.mark.parametrize("B", H.ROWS)
@pytest.mark.parametrize("norm_mul,with_next", [(1, True), (2, True), (2, False)])
def test_td_targets(B, norm_mul, with_next):
    t, d = td_device(B)
    B_norm, what = norm_mul * B, "B%d norm%d next%d" % (B, norm_mul, with_next)
    mul = H.f32(1.0 / B_norm)
    fn = lambda q: H.td_targets(q, H.GAMMA, B_norm, mul)
    got, part = launch_td_targets(d, B, B_norm, with_next)
    ref, bar = compare("td_targets", fn, H.td_inputs(t), got, what)
    sums_close("td_targets", "partials", part, H.block_sums(ref["e2"]), H.block_sums(bar["e2"]), what)
    if with_next:      # mask 0: the target is the reward itself
        off = t["rcm"][:, H.RCM_COLS["mask"]] == 0
        assert torch.equal(got["next_q"][off], t["rcm"][:, H.RCM_COLS["reward"]][off])
        assert torch.equal(got["next_l"][off], t["rcm"][:, H.RCM_COLS["constraint"]][off])
    # with a ticket the launch finishes the three losses itself
    tk, out = tickets(1), out_buf(1, 3)
    got2, part2 = launch_td_targets(d, B, B_norm, with_next, tk, mul, out)
    assert int(tk.abs().sum().item()) == 0
    same_bits(got2["dq"], got["dq"], "dq with and without the ticket")
    same_bits(part2, part, "partials with and without the ticket")
    compare("td_targets", fn, H.td_inputs(t), dict(losses=read(out, 1, 3, "out")[0]), what + " ticket")


@pytest.mark.parametrize("B", H.ROWS)
@pytest.mark.parametrize("norm_mul,with_next", [(1, True), (2, False)])
def test_td_value(B, norm_mul, with_next):
    t, d = td_device(B)
    B_norm, what, n_blk = norm_mul * B, "B%d norm%d next%d" % (B, norm_mul, with_next), (B + 255) // 256
    mul = H.f32(1.0 / B_norm)
    fn = lambda q: H.td_value(q, H.GAMMA, B_norm, mul)
    res = []
    for tk in (None, tickets(1)):
        dpred, nxt, part, out = out_buf(B), out_buf(B) if with_next else None, out_buf(n_blk), out_buf(1)
        lib().call("nlbac_td_value", d["xt"].data_ptr(), d["xsig"], H.RCM_LD, d["mask"], H.RCM_LD, d["xq"].data_ptr(), H.GAMMA,
                   B, B_norm, dpred.data_ptr(), ptr(nxt), part.data_ptr(), ptr(tk), mul, out.data_ptr(), stream())
        torch.cuda.synchronize()
        got = dict(dpred=read(dpred, B, 1, "dpred")[:, 0])
        if with_next:
            got["next_out"] = read(nxt, B, 1, "next_out")[:, 0]
        if tk is not None:
            assert int(tk.abs().sum().item()) == 0
            got["loss"] = read(out, 1, 1, "out")[0, 0]
        else:
            assert bool(torch.isnan(out.cpu()[0]).all()), "out was written without a ticket"
        ref, bar = compare("td_value", fn, H.td_value_inputs(t), got, what + (" ticket" if tk is not None else ""))
        p = read(part, n_blk, 1, "partials")
        sums_close("td_value", "partials", p, H.block_sums(ref["e2"]), H.block_sums(bar["e2"]), what)
        res.append((got["dpred"], p))
    same_bits(res[0][0], res[1][0], "dpred with and without the ticket")
    same_bits(res[0][1], res[1][1], "partials with and without the ticket")


def exact_branch_gradients(t, B_norm, dq1, dq2, what):
    """Every d min(Q1, Q2) is g, g / 2 or 0 with g = -(1.0f / (float)B_norm): one IEEE division, one exact halving."""
    g = -(np.float32(1.0) / np.float32(B_norm))
    a, b = t["q1"].numpy(), t["q2"].numpy()
    zero, half = np.float32(0.0), np.float32(0.5) * g
    want1 = np.where(a < b, g, np.where(a == b, half, zero)).astype(np.float32)
    want2 = np.where(b < a, g, np.where(a == b, half, zero)).astype(np.float32)
    np.testing.assert_array_equal(dq1.numpy(), want1, what)
    np.testing.assert_array_equal(dq2.numpy(), want2, what)


def actor_device(t):
    """Device copies of the rows, log_alpha spread with its stride among sentinels, and the addresses per problem."""
    d = {k: dev(v) for k, v in t.items() if k != "log_alpha"}
    la = torch.full((2 * H.LOG_ALPHA_STRIDE,), H.SENTINEL)
    la[::H.LOG_ALPHA_STRIDE][:len(t["log_alpha"])] = t["log_alpha"]
    d["la"] = dev(la)
    return d


def actor_args(d, g_la, sc, P):
    F = lib().ActorScalarArgs()
    F.target_entropy, F.sc = H.TARGET_ENTROPY, sc.data_ptr()
    for p in range(P):
        F.log_alpha[p] = d["la"].data_ptr() + 4 * p * H.LOG_ALPHA_STRIDE
        F.g_log_alpha[p] = g_la.data_ptr() + 4 * p * H.LOG_ALPHA_STRIDE
    return F


def read_scalars(sc, g_la, first, P):
    """(dict like ``H.actor_scalars``' of what a launch left in the scalars block and the gradient array, the block)."""
    h, g = sc.cpu(), g_la.cpu()
    out = {k: h[idx] for k, idx in H.sc_slots(first, P).items()}
    out["g_log_alpha"] = g[::H.LOG_ALPHA_STRIDE][:P]
    assert bool(torch.isnan(g.view(-1, H.LOG_ALPHA_STRIDE)[:, 1:]).all()) and bool(torch.isnan(g[::H.LOG_ALPHA_STRIDE][P:]).all())
    return out, h


def scalars_untouched(before, after, first, P, what):
    keep = np.ones(H.SC_SIZE, dtype=bool)
    for idx in H.sc_slots(first, P).values():
        keep[idx] = False
    np.testing.assert_array_equal(after.numpy().view(np.int32)[keep], before.numpy().view(np.int32)[keep], what)


@pytest.mark.parametrize("B", H.ROWS)
@pytest.mark.parametrize("P", [1, 2])
def test_actor_q_terms(B, P):
    fn, t, B_norm = H.actor_q_setup(B, P)
    fn_l, t_l, _ = H.actor_losses_setup(B, P)
    d, what, n_blk = actor_device(t_l), "B%d P%d" % (B, P), (B + 255) // 256
    res = []
    for fused in (False, True):
        dq1, dq2, part = out_buf(P * B), out_buf(P * B), out_buf(P * n_blk, 2)
        sc0 = H.sc_block()
        sc, g_la, tk = dev(sc0), dev(torch.full((2 * H.LOG_ALPHA_STRIDE,), NAN)), tickets(1)
        F = actor_args(d, g_la, sc, P)
        lib().call("nlbac_actor_q_terms", d["q1"].data_ptr(), d["q2"].data_ptr(), d["logp"].data_ptr(), d["alpha"].data_ptr(),
                   B, B_norm, P, dq1.data_ptr(), dq2.data_ptr(), part.data_ptr(), C.byref(F) if fused else None,
                   tk.data_ptr() if fused else None, stream())
        if not fused:       # the scalars from the unfused launch's partials: log_alpha / g_log_alpha with their stride
            lib().call("nlbac_actor_scalars", part.data_ptr(), n_blk, B_norm, 0, P, H.TARGET_ENTROPY, d["la"].data_ptr(),
                       H.LOG_ALPHA_STRIDE, g_la.data_ptr(), sc.data_ptr(), stream())
        torch.cuda.synchronize()
        assert int(tk.abs().sum().item()) == 0
        got = dict(dq1=read(dq1, P * B, 1, "dq1")[:, 0], dq2=read(dq2, P * B, 1, "dq2")[:, 0])
        ref, bar = compare("actor_q", fn, t, got, what + " fused%d" % fused)
        exact_branch_gradients(t, B_norm, got["dq1"], got["dq2"], what)
        p = read(part, P * n_blk, 2, "partials").view(P, n_blk, 2)
        for k in range(P):
            rows = slice(k * B, (k + 1) * B)
            sums_close("actor_q", "partials", p[k], H.block_sums(ref["terms"][rows]), H.block_sums(bar["terms"][rows]), what)
        scal, after = read_scalars(sc, g_la, 0, P)
        compare("actor_losses", fn_l, t_l, scal, what + " fused%d" % fused)
        scalars_untouched(sc0, after, 0, P, what)
        res.append((got["dq1"], got["dq2"], p, after, g_la.cpu()))
    # "same sums in the same order": the fused launch == the unfused one + nlbac_actor_scalars, bit for bit
    for x, y, name in zip(res[0], res[1], ("dq1", "dq2", "partials", "scalars", "g_log_alpha")):
        assert torch.equal(torch.nan_to_num(x, nan=7.0).view(I32), torch.nan_to_num(y, nan=7.0).view(I32)), name


@pytest.mark.parametrize("n_blk", [1, 3])
@pytest.mark.parametrize("first,P", H.SCALARS_VARIANTS)
def test_actor_scalars_and_alpha_refresh(n_blk, first, P):
    t = H.scalars_inputs(n_blk, first, P)
    d, what = actor_device(t), "blk%d first%d P%d" % (n_blk, first, P)
    d_part = dev(t["partials"])
    sc0 = H.sc_block()
    sc, g_la = dev(sc0), dev(torch.full((2 * H.LOG_ALPHA_STRIDE,), NAN))
    B = 256 * n_blk
    lib().call("nlbac_actor_scalars", d_part.data_ptr(), n_blk, B, first, P, H.TARGET_ENTROPY, d["la"].data_ptr(),
               H.LOG_ALPHA_STRIDE, g_la.data_ptr(), sc.data_ptr(), stream())
    torch.cuda.synchronize()
    got, after = read_scalars(sc, g_la, first, P)
    compare("actor_scalars", lambda q: H.actor_scalars(q, float(B), first, P, H.TARGET_ENTROPY), t, got, what)
    scalars_untouched(sc0, after, first, P, what)
    lib().call("nlbac_alpha_refresh", d["la"].data_ptr(), H.LOG_ALPHA_STRIDE, first, P, sc.data_ptr(), stream())
    torch.cuda.synchronize()
    last = sc.cpu()
    compare("alpha_refresh", lambda q: H.alpha_refresh(dict(log_alpha=q["log_alpha"])), t,
            dict(alpha=last[H.SC_ALPHA + first:H.SC_ALPHA + first + P]), what)
    keep = np.ones(H.SC_SIZE, dtype=bool)
    keep[H.SC_ALPHA + first:H.SC_ALPHA + first + P] = False
    np.testing.assert_array_equal(last.numpy().view(np.int32)[keep], after.numpy().view(np.int32)[keep])


@pytest.mark.parametrize("n", H.ROWS)
@pytest.mark.parametrize("d,extra,norm_mul", H.MSE_SHAPES)
def test_mse_forward_backward(n, d, extra, norm_mul):
    t, g = H.mse_case(n, d), H.gen(120 + n)
    (pred, pred_ld), (target, target_ld) = wide(t["pred"], extra, g), wide(t["target"], extra + 1, g)
    n_blk, what = (n + 255) // 256, "n%d d%d norm%d" % (n, d, norm_mul)
    dpred, part = out_buf(n, d + 2), out_buf(n_blk)
    lib().call("nlbac_mse_fwd_bwd", pred.data_ptr(), pred_ld, target.data_ptr(), target_ld, n, norm_mul * n, d,
               dpred.data_ptr(), d + 2, part.data_ptr(), stream())
    torch.cuda.synchronize()
    ref, bar = compare("mse", lambda q: H.mse(q, norm_mul * n), t, dict(dpred=read(dpred, n, d, "dpred")), what)
    sums_close("mse", "partials", read(part, n_blk, 1, "partials"), H.block_sums(ref["e2"]), H.block_sums(bar["e2"]), what)


# ---------------------------------------------------------------------------
# B. the heads fused into the MLP launches, per kernel family
# ---------------------------------------------------------------------------
FAMILIES = {"tiled": 96, "half-panel": 64, "quarter-panel": 128}        # 3-layer nets of this width (mlp_family, mlp_launch.h)
TILE = {"tiled": 32, "half-panel": 32, "quarter-panel": 16}
IN_DIM = 7
BATCHES = H.HEAD_BATCHES


def shape_policy_outputs(mods, n_u):
    """Scale the last layers so that the heads reach the regimes of ``heads_common``: log_std columns with a spread of
    about 10 around -5 (both sides of the clamp), mean columns with a spread of about 3 (tanh saturates on many rows);
    (net, log_std column) pairs in turn get zero weights and a bias of exactly 2.0, of exactly -20.0 (with the mean of that
    column exactly 0, so that x - mean is exact), or stay free."""
    x = torch.randn(256, IN_DIM, generator=H.gen(7))
    with torch.no_grad():
        for i, m in enumerate(mods):
            h = torch.relu(m[1](torch.relu(m[0](x))))
            spread = m[2](h).std(0)
            last = m[2]
            for c in range(n_u):
                last.weight[c] *= 3.0 / spread[c]
                last.weight[n_u + c] *= 10.0 / spread[n_u + c]
                last.bias[n_u + c] = -5.0
                turn = (i * n_u + c) % 3
                if turn < 2:
                    last.weight[n_u + c] = 0.0
                    last.bias[n_u + c] = (2.0, -20.0)[turn]
                if turn == 1:
                    last.weight[c] = 0.0
                    last.bias[c] = 0.0


@functools.lru_cache(maxsize=None)
def nets_of(family, n_nets, out_dim, policy=False):
    """``n_nets`` 3-layer nets of the family's width in one arena, packed; policy nets get their last layers shaped."""
    from nlbac_amd import arena as A
    hid = FAMILIES[family]
    torch.manual_seed(1000 + 10 * hid + n_nets + out_dim)
    mods = [[nn.Linear(IN_DIM, hid), nn.Linear(hid, hid), nn.Linear(hid, out_dim)] for _ in range(n_nets)]
    for m in mods:
        for l in m:
            nn.init.uniform_(l.bias, -0.3, 0.3)
    if policy:
        shape_policy_outputs(mods, out_dim // 2)
    ar = A.Arena("cuda", n_slabs=1)
    hs = [A.MlpHandle(ar, [(l.weight, l.bias) for l in m]) for m in mods]
    ar.finalize()
    for h in hs:
        h.bind()
    A.pack(hs)
    nets = A.mlp_array([h.desc for h in hs])
    panel = lib().load().nlbac_mlp_masks_ok(nets, n_nets)
    quarter = lib().load().nlbac_mlp_fwd_head_ok(nets, n_nets)
    assert (panel, quarter) == {"tiled": (0, 0), "half-panel": (1, 0), "quarter-panel": (1, 1)}[family]
    return types.SimpleNamespace(arena=ar, handles=hs, nets=nets, n=n_nets, hid=hid, out_dim=out_dim, family=family)


def make_io(N, B, x, dy=None):
    """An io array over the shared input rows ``x`` (B, IN_DIM): per net y (ld out_dim + 1), acts, dz, dx — NaN prefilled,
    y and dx with a guard row; ``dy``: per net (device tensor, ld) for the plain data backward."""
    from nlbac_amd import arena as A
    io, bufs = A.io_array(N.n), []
    for i in range(N.n):
        b = types.SimpleNamespace(y=out_buf(B, N.out_dim + 1), acts=torch.full((2, B, N.hid), NAN, device="cuda"),
                                  dz=torch.full((2, B, N.hid), NAN, device="cuda"), dx=out_buf(B, IN_DIM + 1))
        io[i].x0, io[i].x0_dim, io[i].x0_ld = x.data_ptr(), IN_DIM, IN_DIM
        io[i].y, io[i].y_ld = b.y.data_ptr(), N.out_dim + 1
        io[i].acts, io[i].dz = b.acts.data_ptr(), b.dz.data_ptr()
        io[i].dx, io[i].dx_ld = b.dx.data_ptr(), IN_DIM + 1
        if dy is not None:
            io[i].dy, io[i].dy_ld = dy[i][0].data_ptr(), dy[i][1]
        bufs.append(b)
    return io, bufs


def forward(N, B, seed):
    """x on the device and an io array whose acts a plain forward has filled."""
    x = dev(torch.randn(B, IN_DIM, generator=H.gen(seed)))
    io, bufs = make_io(N, B, x)
    lib().call("nlbac_mlp_fwd", N.nets, io, N.n, B, stream())
    return x, io, bufs


def same_backward(N, B, x, bufs, dy, what):
    """dz / dx of the head launch (``bufs``) == those of ``nlbac_mlp_bwd_data`` fed dy = the head's row output."""
    io2, bufs2 = make_io(N, B, x, dy)
    for i in range(N.n):                # (the activations the forward left, which the head launch gated with too)
        io2[i].acts = bufs[i].acts.data_ptr()
    lib().call("nlbac_mlp_bwd_data", N.nets, io2, N.n, B, stream())
    torch.cuda.synchronize()
    for i, (b, b2) in enumerate(zip(bufs, bufs2)):
        assert bool(torch.isfinite(b.dz).all()), "%s: dz of net %d" % (what, i)
        same_bits(b.dz, b2.dz, "%s: dz of net %d against the plain data backward" % (what, i))
        same_bits(read(b.dx, B, IN_DIM, "dx"), read(b2.dx, B, IN_DIM, "dx"), "%s: dx of net %d" % (what, i))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_nets,n_u", [(1, 1), (1, 4), (3, 1), (3, 2), (3, 4), (1, 2)])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_forward_with_the_gauss_head(family, n_nets, n_u, B):
    N = nets_of(family, n_nets, 2 * n_u, True)
    g = H.gen(200 + B + n_u)
    n, what = n_nets * B, "%s nets%d nu%d B%d" % (family, n_nets, n_u, B)
    eps = torch.randn(n, n_u, generator=g)
    eps[::5] = 0.0
    scale, bias = 0.5 + 1.5 * torch.rand(n_u, generator=g), 0.25 + torch.rand(n_u, generator=g)
    x = dev(torch.randn(B, IN_DIM, generator=g))
    io, bufs = make_io(N, B, x)
    d_eps, d_scale, d_bias = dev(eps), dev(scale), dev(bias)
    action, logp = out_buf(n, n_u + 2), out_buf(n)
    G = lib().GaussHead()
    G.eps, G.scale, G.bias, G.n_u = d_eps.data_ptr(), d_scale.data_ptr(), d_bias.data_ptr(), n_u
    G.action, G.action_ld, G.logp = action.data_ptr(), n_u + 2, logp.data_ptr()
    lib().call("nlbac_mlp_fwd_gauss", N.nets, io, n_nets, B, C.byref(G), stream())
    torch.cuda.synchronize()
    # the reference's input is the y the launch itself wrote: the head is under test, not the MLP
    y = torch.cat([read(b.y, B, 2 * n_u, "y") for b in bufs])
    assert bool(torch.isfinite(y).all())
    t = dict(heads=y, eps=eps, scale=scale, bias=bias)
    a, lp = read(action, n, n_u, "action"), read(logp, n, 1, "logp")[:, 0]
    check_gauss_fwd(t, n_u, a, lp, what)
    reg = H.heads_regimes_of(y, eps, n_u)
    if n_nets * n_u >= 2:       # the columns pinned to the clamp's boundaries sit there in every row
        assert int(reg["at_max"].sum()) >= B and int(reg["at_min"].sum()) >= B
    a2, lp2 = launch_gauss_fwd(dev(y), 2 * n_u, d_eps, d_scale, d_bias, n_u, n)
    same_bits(a, a2, what + ": action against nlbac_gauss_sample_fwd on the same y")
    same_bits(lp, lp2, what + ": logp against nlbac_gauss_sample_fwd on the same y")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_nets,with_dheads", [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_with_the_gauss_head(family, n_nets, with_dheads, B):
    n_u, n_src, P, norm_mul = H.GAUSS_HEAD_VARIANTS[n_nets - 1]
    N = nets_of(family, n_nets, 2 * n_u)
    fn, t, noise, B_norm, mul = H.gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
    n, what = n_nets * B, "%s nets%d dheads%d B%d" % (family, n_nets, with_dheads, B)
    d = gauss_bwd_device(t, n_u, 300 + B)
    rows = launch_gauss_bwd(d, t, n_u, n, B, mul)           # the per-row entry point on the same arrays
    x, io, bufs = forward(N, B, 310 + B)
    dheads = out_buf(n, 2 * n_u + 1)
    Hd = lib().DyHead()
    Hd.kind, Hd.B_norm, Hd.n_u = 1, B_norm, n_u
    Hd.heads, Hd.heads_ld, Hd.eps, Hd.scale = d["heads"].data_ptr(), d["heads_ld"], d["eps"].data_ptr(), d["scale"].data_ptr()
    for k in range(n_src):
        Hd.da[k], Hd.da_ld[k] = d["da%d" % k].data_ptr(), t["da%d" % k].shape[1]
    Hd.alpha, Hd.dlogp_mul = d["alpha"].data_ptr(), mul
    if with_dheads:
        Hd.dheads, Hd.dheads_ld = dheads.data_ptr(), 2 * n_u + 1
    lib().call("nlbac_mlp_bwd_data_head", N.nets, io, n_nets, B, C.byref(Hd), stream())
    torch.cuda.synchronize()
    if with_dheads:
        got = read(dheads, n, 2 * n_u, "dheads")
        check_gauss_bwd(fn, t, noise, n_u, got, what)
        same_bits(got, rows, what + ": dheads against nlbac_gauss_sample_bwd")
    else:
        assert bool(torch.isnan(dheads.cpu()[:n]).all())
    d_rows = dev(rows)
    same_backward(N, B, x, bufs, [(d_rows[i * B:], 2 * n_u) for i in range(n_nets)], what)


def td_head(d, B, B_norm, n_nets, mul, o):
    """The kind-2 head over a ``td_device`` case; ``o``: its output buffers."""
    Hd = lib().DyHead()
    Hd.kind, Hd.B_norm, Hd.gamma, Hd.mul = 2, B_norm, H.GAMMA, mul
    Hd.q1t, Hd.q2t, Hd.lt, Hd.nlogp = (d[k].data_ptr() for k in ("q1t", "q2t", "lt", "nlogp"))
    Hd.reward, Hd.constraint, Hd.mask, Hd.rcm_ld, Hd.alpha = d["reward"], d["constraint"], d["mask"], H.RCM_LD, d["alpha"].data_ptr()
    for k, name in enumerate(("q1", "q2", "lf")):
        Hd.q[k], Hd.dq[k] = d[name].data_ptr(), o.dq[k].data_ptr()
    Hd.next_q, Hd.next_l = o.next_q.data_ptr(), o.next_l.data_ptr()
    Hd.partials, Hd.ticket, Hd.out = o.partials.data_ptr(), o.tickets.data_ptr(), o.out.data_ptr()
    if n_nets == 4:
        Hd.xt, Hd.xsig, Hd.xsig_ld, Hd.xq = d["xt"].data_ptr(), d["xsig"], H.RCM_LD, d["xq"].data_ptr()
        Hd.dxq, Hd.out_x = o.dxq.data_ptr(), o.out_x.data_ptr()
    return Hd


def td_outputs(B, n_nets):
    n_tiles = (B + 15) // 16
    return types.SimpleNamespace(dq=[out_buf(B) for _ in range(3)], next_q=out_buf(B), next_l=out_buf(B), dxq=out_buf(B),
                                 partials=out_buf(n_tiles * n_nets), tickets=tickets(1 + (n_nets * n_tiles + 15) // 16),
                                 out=out_buf(1, 3), out_x=out_buf(1), sums_tiles=tickets(2))


def read_td(o, B, n_nets):
    got = dict(dq=torch.cat([read(b, B, 1, "dq") for b in o.dq], 1), next_q=read(o.next_q, B, 1, "next_q")[:, 0],
               next_l=read(o.next_l, B, 1, "next_l")[:, 0], losses=read(o.out, 1, 3, "out")[0])
    if n_nets == 4:
        got.update(dpred=read(o.dxq, B, 1, "dxq")[:, 0], loss=read(o.out_x, 1, 1, "out_x")[0, 0])
    return got


def check_td_head(family, n_nets, B, norm_mul):
    N = nets_of(family, n_nets, 1)
    t, d = td_device(B)
    B_norm, what = norm_mul * B, "%s nets%d B%d norm%d" % (family, n_nets, B, norm_mul)
    mul = H.f32(1.0 / B_norm)
    x, io, bufs = forward(N, B, 400 + B)
    o = td_outputs(B, n_nets)
    Hd = td_head(d, B, B_norm, n_nets, mul, o)
    lib().call("nlbac_mlp_bwd_data_head", N.nets, io, n_nets, B, C.byref(Hd), stream())
    torch.cuda.synchronize()
    assert int(o.tickets.abs().sum().item()) == 0
    got = read_td(o, B, n_nets)
    compare("td_targets", lambda q: H.td_targets(q, H.GAMMA, B_norm, mul), H.td_inputs(t),
            {k: got[k] for k in ("dq", "next_q", "next_l", "losses")}, what)
    rows, _ = launch_td_targets(d, B, B_norm, True)
    for k in ("dq", "next_q", "next_l"):
        same_bits(got[k], rows[k], what + ": %s against nlbac_td_targets" % k)
    dy = [(dev(got["dq"][:, k].contiguous()), 1) for k in range(3)]
    if n_nets == 4:
        compare("td_value", lambda q: H.td_value(q, H.GAMMA, B_norm, mul), H.td_value_inputs(t),
                dict(dpred=got["dpred"], loss=got["loss"]), what)
        dpred, part = out_buf(B), out_buf((B + 255) // 256)
        lib().call("nlbac_td_value", d["xt"].data_ptr(), d["xsig"], H.RCM_LD, d["mask"], H.RCM_LD, d["xq"].data_ptr(), H.GAMMA,
                   B, B_norm, dpred.data_ptr(), None, part.data_ptr(), None, mul, None, stream())
        torch.cuda.synchronize()
        same_bits(got["dpred"], read(dpred, B, 1, "dpred")[:, 0], what + ": dxq against nlbac_td_value")
        dy.append((dev(got["dpred"]), 1))
    else:
        assert bool(torch.isnan(o.dxq.cpu()[:B]).all()) and bool(torch.isnan(o.out_x.cpu()[0]).all())
    same_backward(N, B, x, bufs, dy, what)
    return got


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_nets", [3, 4])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_with_the_td_head(family, n_nets, B):
    check_td_head(family, n_nets, B, H.head_norm_mul(B))


def test_td_head_sums_257_tiles_of_the_quarter_panel_family():
    """B = 4112 = 257 tiles of 16 rows: the elected workgroup's threads take tiles t, t + 256 (``elected_tile_sums``)."""
    check_td_head("quarter-panel", 3, H.MANY_TILES, 1)


def actor_head(d, B_norm, P, o):
    Hd = lib().DyHead()
    Hd.kind, Hd.B_norm, Hd.n_prob = 3, B_norm, P
    Hd.qa, Hd.qb, Hd.logp, Hd.alpha = (d[k].data_ptr() for k in ("q1", "q2", "logp", "alpha"))
    Hd.dqa, Hd.dqb = o.dqa.data_ptr(), o.dqb.data_ptr()
    F = actor_args(d, o.g_la, o.sc, P)
    C.memmove(C.byref(Hd.actor), C.byref(F), C.sizeof(F))
    Hd.partials, Hd.ticket = o.partials.data_ptr(), o.tickets.data_ptr()
    return Hd


def actor_outputs(B, P):
    n_tiles = (B + 15) // 16
    sc0 = H.sc_block()
    return types.SimpleNamespace(dqa=out_buf(P * B), dqb=out_buf(P * B), partials=out_buf(2 * P * n_tiles), sc0=sc0, sc=dev(sc0),
                                 tickets=tickets(1 + (P * n_tiles + 15) // 16), sums_tiles=tickets(2),
                                 g_la=dev(torch.full((2 * H.LOG_ALPHA_STRIDE,), NAN)))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_with_the_actor_head(family, P, B):
    N = nets_of(family, 2 * P, 1)
    fn, t, B_norm = H.actor_q_setup(B, P)
    fn_l, t_l, _ = H.actor_losses_setup(B, P)
    d, what = actor_device(t_l), "%s P%d B%d" % (family, P, B)
    x, io, bufs = forward(N, B, 500 + B)
    o = actor_outputs(B, P)
    Hd = actor_head(d, B_norm, P, o)
    lib().call("nlbac_mlp_bwd_data_head", N.nets, io, 2 * P, B, C.byref(Hd), stream())
    torch.cuda.synchronize()
    assert int(o.tickets.abs().sum().item()) == 0
    got = dict(dq1=read(o.dqa, P * B, 1, "dqa")[:, 0], dq2=read(o.dqb, P * B, 1, "dqb")[:, 0])
    compare("actor_q", fn, t, got, what)
    exact_branch_gradients(t, B_norm, got["dq1"], got["dq2"], what)
    scal, after = read_scalars(o.sc, o.g_la, 0, P)
    compare("actor_losses", fn_l, t_l, scal, what)
    scalars_untouched(o.sc0, after, 0, P, what)
    # net i = (controller i / 2, Q1 / Q2 = i % 2): its dy are rows (i / 2) B .. of dqa / dqb
    d1, d2 = dev(got["dq1"]), dev(got["dq2"])
    same_backward(N, B, x, bufs, [((d1, d2)[i % 2][(i // 2) * B:], 1) for i in range(2 * P)], what)


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_deferred_sums_finished_by_a_later_launch(family, kind):
    """``sums_defer``: the head's launch leaves its tile partials and the tile count; a job of a later kind-1 launch
    finishes them — the same sums in the same order as the elected workgroup's, so the outputs agree bit for bit."""
    B, n_u = 600, 2
    NP = nets_of(family, 1, 2 * n_u)
    fn, tg, noise, _, mul_g = H.gauss_bwd_setup(B, n_u, 1, 1, 1)
    dg = gauss_bwd_device(tg, n_u, 600)
    if kind == 2:
        n_nets = 3
        N = nets_of(family, n_nets, 1)
        t, d = td_device(B)
        mul = H.f32(1.0 / B)
        outs = [td_outputs(B, n_nets) for _ in range(2)]
        heads = [td_head(d, B, B, n_nets, mul, o) for o in outs]
    else:
        n_nets = 4
        N = nets_of(family, n_nets, 1)
        _, t_l, B_norm = H.actor_losses_setup(B, 2)
        d = actor_device(t_l)
        outs = [actor_outputs(B, 2) for _ in range(2)]
        heads = [actor_head(d, B_norm, 2, o) for o in outs]
    x, io, bufs = forward(N, B, 610)
    lib().call("nlbac_mlp_bwd_data_head", N.nets, io, n_nets, B, C.byref(heads[0]), stream())      # the elected run
    Hd, o = heads[1], outs[1]
    Hd.sums_defer, Hd.sums_tiles = 1, o.sums_tiles.data_ptr()
    io1, bufs1 = make_io(N, B, x)
    for i in range(n_nets):
        io1[i].acts = bufs[i].acts.data_ptr()
    lib().call("nlbac_mlp_bwd_data_head", N.nets, io1, n_nets, B, C.byref(Hd), stream())
    torch.cuda.synchronize()
    n_tiles = (B + TILE[family] - 1) // TILE[family]
    assert o.sums_tiles.cpu().tolist() == [n_tiles, 0]
    assert int(o.tickets.abs().sum().item()) == 0
    if kind == 2:       # nothing finished yet
        assert bool(torch.isnan(o.out.cpu()[0]).all())
    else:
        assert torch.equal(o.sc.cpu().view(I32), o.sc0.view(I32)) and bool(torch.isnan(o.g_la.cpu()).all())
    # the later launch: one policy net, kind 1, with the job
    xp, iop, bufsp = forward(NP, B, 620)
    G = lib().DyHead()
    G.kind, G.B_norm, G.n_u = 1, B, n_u
    G.heads, G.heads_ld, G.eps, G.scale = dg["heads"].data_ptr(), dg["heads_ld"], dg["eps"].data_ptr(), dg["scale"].data_ptr()
    G.da[0], G.da_ld[0] = dg["da0"].data_ptr(), tg["da0"].shape[1]
    G.alpha, G.dlogp_mul = dg["alpha"].data_ptr(), mul_g
    J = G.finish[0]
    J.kind, J.partials, J.n_tiles = kind, Hd.partials, Hd.sums_tiles
    if kind == 2:
        J.n_nets, J.mul, J.out = n_nets, Hd.mul, Hd.out
    else:
        J.n_nets, J.B_norm = 2, Hd.B_norm
        C.memmove(C.byref(J.actor), C.byref(Hd.actor), C.sizeof(Hd.actor))
    lib().call("nlbac_mlp_bwd_data_head", NP.nets, iop, 1, B, C.byref(G), stream())
    torch.cuda.synchronize()
    if kind == 2:
        a, b = read_td(outs[0], B, n_nets), read_td(o, B, n_nets)
        for k in a:
            same_bits(a[k], b[k], "%s: %s, deferred against elected" % (family, k))
    else:
        same_bits(outs[0].sc.cpu(), o.sc.cpu(), "%s: scalars, deferred against elected" % family)
        same_bits(torch.nan_to_num(outs[0].g_la.cpu(), nan=7.0), torch.nan_to_num(o.g_la.cpu(), nan=7.0), "g_log_alpha")
        assert not torch.equal(o.sc.cpu().view(I32), o.sc0.view(I32))
        for k in ("dqa", "dqb"):
            same_bits(getattr(outs[0], k).cpu(), getattr(o, k).cpu(), k)
    for b0, b1 in zip(bufs, bufs1):
        same_bits(b0.dz, b1.dz, "dz, deferred against elected")
