"""The optimiser step, the streaming helpers and the device-side draw (``csrc/optim_kernels.hip``, ``csrc/philox.h``,
``nlbac_sample_rows_head``), each entry point launched on its own through the C ABI on hand-made tensors and held to the
references of ``optim_common``: bit patterns where the operation is exact (slab sums, copies, gathers, the draw's
indices, one launch against another), the float64 reference and bar (``K`` fixed on the CPU, see there) and
``vec_close(..., 1e-4)`` where it rounds.  Every output buffer is a little longer than what the kernel owns and ends in
sentinels that must survive bit for bit.  Each check prints its device / bar ratio before it asserts.  Nothing here
launches with a bad pointer, a misaligned table or an out-of-range size: those are the host file's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_common as O
import task_kernels_common as T
from common import vec_close

pytestmark = pytest.mark.gpu
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
SENT = O.SENT
GUARD = 8
STATE_GUARD = 0x5A5A5A5A


def lib():
    from nlbac_amd import _lib
    return _lib


def stream():
    from nlbac_amd.arena import stream_ptr
    return stream_ptr()


def call(name, *args):
    lib().call(name, *(args + (stream(),)))


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def same(a, b):
    """Equal bit for bit (NaNs and signed zeros included)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(x):
    """``x`` (host, flat) on the device, padded to a multiple of four and followed by GUARD sentinels."""
    x = torch.as_tensor(x).reshape(-1)
    buf = torch.full((O.round4(x.numel()) + GUARD,), SENT, dtype=F32)
    buf[:x.numel()] = x
    return buf.cuda()


def unguard(buf, n, what):
    """The n floats the kernel owns, after checking that it wrote nothing behind them."""
    h = buf.cpu().reshape(-1)
    assert same(h[n:], torch.full_like(h[n:], SENT)), "%s: written past its end" % what
    return h[:n].clone()


def state_block(step):
    """AdamState {step, step_size, bc2_sqrt, ticket = 0} with stale floats, and a guard behind it."""
    st = torch.full((8,), STATE_GUARD, dtype=torch.int32)
    st[0], st[3] = step, 0
    st[1:3] = bits(torch.tensor([SENT, SENT]))
    return st.cuda()


def check_state(st, t, what=""):
    """step == t, ticket == 0, the floats within one float32 ulp of the Python doubles; -> (step_size, bc2_sqrt)."""
    h = st.cpu()
    assert int(h[0]) == t and int(h[3]) == 0, "%s: step / ticket %d / %d, expected %d / 0" % (what, h[0], h[3], t)
    assert bool((h[4:] == STATE_GUARD).all()), "%s: written past the state block" % what
    ss, bc = (float(x) for x in h[1:3].clone().view(F32))
    want = O.step_consts(O.LR, t)
    assert O.ulp_close(ss, want[0]) and O.ulp_close(bc, want[1]), "%s: step %d constants %r, expected %r" % (what, t, (ss, bc), want)
    return ss, bc


def fused(d, g_ptr, n_slabs, stride, n, st, tau, tg, scatter=None, scatter_target=None, slots=2, alpha=None, mirror=None):
    n_al = len(alpha[0]) if alpha else 0
    al_off = (C.c_long * 2)(*(list(alpha[0]) + [0, 0])[:2]) if alpha else None
    al_dst = (C.c_void_p * 2)(*(list(alpha[1]) + [None, None])[:2]) if alpha else None
    ms, md, nm = mirror if mirror else (None, None, 0)
    call("nlbac_adam_fused", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), g_ptr, n_slabs, stride, n,
         st.data_ptr(), O.LR, ptr(tg), tau, ptr(scatter), ptr(scatter_target), slots, n_al, al_off, al_dst, ms, md, nm)


def run_adam(c, how, tau=O.TAU, target=True, inputs=None, grad=None, **kw):
    """One optimiser step of case ``c``: ``how`` = "fused" (one launch), "split" (nlbac_adam_prepare + nlbac_adam_step)
    or "dp" (nlbac_reduce_slabs, then nlbac_adam_fused on the one reduced slab: the data-parallel path of ``_adam``).
    -> (p, m, v [, target] on the host, the state block)."""
    x = c.inputs if inputs is None else inputs
    n = c.n
    d = {k: guarded(x[k]) for k in ("p", "m", "v")}
    tg = guarded(x["target"]) if target else None
    gr = guarded((c.grad if grad is None else grad).reshape(-1))
    st = state_block(c.t - 1)
    xb = None
    if how == "split":
        call("nlbac_adam_prepare", st.data_ptr(), O.LR)
        call("nlbac_adam_step", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), gr.data_ptr(), c.n_slabs,
             c.stride, n, st.data_ptr(), ptr(tg), tau)
    elif how == "dp":
        xb = guarded(torch.full((n,), NAN))
        call("nlbac_reduce_slabs", xb.data_ptr(), gr.data_ptr(), c.n_slabs, c.stride, n)
        fused(d, xb.data_ptr(), 1, O.round4(n), n, st, tau, tg, **kw)
    else:
        fused(d, gr.data_ptr(), c.n_slabs, c.stride, n, st, tau, tg, **kw)
    torch.cuda.synchronize()
    out = {k: unguard(d[k], n, "%s (%s, %s)" % (k, how, c.label)) for k in d}
    if tg is not None:
        out["target"] = unguard(tg, n, "target (%s, %s)" % (how, c.label))
    if xb is not None:
        unguard(xb, n, "reduced slab")
    return out, st.cpu()


def same_run(a, b, what):
    (oa, sa), (ob, sb) = a, b
    assert set(oa) == set(ob)
    for k in oa:
        assert same(oa[k], ob[k]), "%s: %s differs in %d of %d elements" % (
            what, k, int((bits(oa[k]) != bits(ob[k])).sum()), oa[k].numel())
    assert torch.equal(sa, sb), "%s: the state blocks differ: %s / %s" % (what, sa.tolist(), sb.tolist())


def adam_ratios(key, out, consts, tau, what):
    """device / bar per output against the float64 reference (not yet asserted)."""
    ref, bar = O.adam_reference(key, consts[0], consts[1], tau)
    assert set(out) == set(ref)
    return {k: (T.bar_ratio(out[k].numpy(), ref[k], O.K["adam_" + k] * bar[k]), what, out[k], ref[k]) for k in out}


def hold(ratios):
    """Print each figure, then assert: inside the bar, and vec_close 1e-4."""
    for r in ratios:
        for k, (v, what, _, _) in r.items():
            print("device / bar  adam_%-7s %-60s %.3f" % (k, what, v))
    for r in ratios:
        for k, (v, what, got, ref) in r.items():
            assert v <= 1.0, "adam %s (%s): %.3f of the bar (K = %d)" % (k, what, v, O.K["adam_" + k])
            vec_close(got.numpy(), ref.numpy(), 1e-4, "adam %s (%s)" % (k, what))


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.ADAM_N)
def test_adam_against_float64_and_its_other_forms(n):
    """nlbac_adam_fused against the float64 reference; nlbac_adam_prepare + nlbac_adam_step and the data-parallel form
    (nlbac_reduce_slabs, then one slab) against it bit for bit: all three run adam_one on slabs added in slab order."""
    ratios = []
    for c in [c for c in O.adam_cases() if c.n == n]:
        one = run_adam(c, "fused")
        consts = check_state(one[1], c.t, c.label)
        ratios.append(adam_ratios(c.key, one[0], consts, O.TAU, c.label))
        same_run(one, run_adam(c, "split"), "prepare + step against fused (%s)" % c.label)
        same_run(one, run_adam(c, "dp"), "reduce_slabs + fused(n_slabs = 1) against fused(n_slabs = %d) (%s)" % (c.n_slabs, c.label))
    hold(ratios)


@pytest.mark.parametrize("how", ["fused", "split"])
def test_adam_three_steps_in_a_row(how):
    """Steps 8, 9, 10 on the same buffers from a counter preset to 7: each step against the float64 step from the
    state the device itself left, and the counter moves by one per launch."""
    c = O.adam_case(1028, 5, 8, 8, 1.0)
    d = {k: guarded(c.inputs[k]) for k in ("p", "m", "v", "target")}
    gr, st = guarded(c.grad.reshape(-1)), state_block(7)
    prev, ratios = dict(c.inputs), []
    for t in (8, 9, 10):
        if how == "fused":
            fused(d, gr.data_ptr(), c.n_slabs, c.stride, c.n, st, O.TAU, d["target"])
        else:
            call("nlbac_adam_prepare", st.data_ptr(), O.LR)
            call("nlbac_adam_step", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), gr.data_ptr(), c.n_slabs,
                 c.stride, c.n, st.data_ptr(), d["target"].data_ptr(), O.TAU)
        torch.cuda.synchronize()
        ss, bc = check_state(st, t, "step %d" % t)
        out = {k: unguard(d[k], c.n, k) for k in d}
        ref, bar = T.reference_and_bar("adam", lambda q: O.adam(q, ss, bc, O.TAU), prev, seed=t, k=1)
        ratios.append({k: (T.bar_ratio(out[k].numpy(), ref[k], O.K["adam_" + k] * bar[k]), "%s step %d" % (how, t), out[k],
                           ref[k]) for k in out})
        prev = dict(prev, **out)
    hold(ratios)


@pytest.mark.parametrize("how", ["fused", "split"])
def test_adam_tau_edges_and_missing_target(how):
    for key in ((5, 4, 0, 2, 1.0), (1023, 2, 8, 2, 1.0)):
        c = O.adam_case(*key)
        base, st = run_adam(c, how)
        for tau in (1.0, 0.0, -1.0):
            out, st2 = run_adam(c, how, tau=tau)
            assert torch.equal(st, st2)
            for k in ("p", "m", "v"):
                assert same(out[k], base[k]), "tau = %g moved %s (%s)" % (tau, k, c.label)
            want = out["p"] if tau == 1.0 else c.inputs["target"]     # tau = 1: target == p; 0: unchanged; < 0: untouched
            assert same(out["target"], want), "tau = %g: target (%s, %s)" % (tau, how, c.label)
        for tau in (O.TAU, -1.0):       # no target at all
            out, st2 = run_adam(c, how, tau=tau, target=False)
            assert torch.equal(st, st2) and set(out) == {"p", "m", "v"}
            for k in out:
                assert same(out[k], base[k]), "a null target moved %s (%s)" % (k, c.label)
            consts = check_state(st2, c.t)
        hold([adam_ratios(c.key, {k: base[k] for k in ("p", "m", "v")}, consts, None, "no target, " + c.label)])


def test_adam_grid_stride_trip():
    """n = 2048 256 4 + 4 256 + 3: the float4 loops take a second trip.  The step is elementwise, so one launch over the
    whole vector equals, bit for bit, the same prepared state applied in chunk launches of at most 2^20 elements; the
    fused entry equals both.  (No float64 reference at this size.)"""
    n, n_slabs = O.ADAM_BIG_N, 2
    stride = O.round4(n) + 8
    g = T.gen(77)
    grad = torch.full((n_slabs, stride), NAN)
    grad[:, :n] = torch.randn(n_slabs, n, generator=g)
    x = dict(p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.3, v=torch.rand(n, generator=g),
             target=torch.randn(n, generator=g))
    gr = guarded(grad.reshape(-1))
    runs = {}
    for how in ("whole", "chunks", "fused"):
        d = {k: guarded(x[k]) for k in x}
        st = state_block(41)
        if how == "fused":
            fused(d, gr.data_ptr(), n_slabs, stride, n, st, O.TAU, d["target"])
        else:
            call("nlbac_adam_prepare", st.data_ptr(), O.LR)
            step = (n,) if how == "whole" else (1 << 20, 1 << 20, n - (2 << 20))
            off = 0
            for m in step:
                assert 1 <= m <= max(n * (how == "whole"), 1 << 20) and off % 4 == 0
                call("nlbac_adam_step", *[d[k].data_ptr() + 4 * off for k in ("p", "m", "v")], gr.data_ptr() + 4 * off,
                     n_slabs, stride, m, st.data_ptr(), d["target"].data_ptr() + 4 * off, O.TAU)
                off += m
            assert off == n
        torch.cuda.synchronize()
        check_state(st, 42, how)
        runs[how] = ({k: unguard(d[k], n, "%s (%s)" % (k, how)) for k in d}, st.cpu())
    assert not same(runs["whole"][0]["p"], x["p"]) and not same(runs["whole"][0]["target"], x["target"])
    same_run(runs["whole"], runs["chunks"], "one nlbac_adam_step launch against chunk launches")
    same_run(runs["whole"], runs["fused"], "nlbac_adam_fused against nlbac_adam_step at the grid-stride size")


def table_for(index, buf):
    """The scatter table of ``optim_common.scatter_layout``'s index into the device float buffer ``buf``."""
    addr = np.where(index >= 0, buf.data_ptr() + 4 * index, 0).astype(np.uint64)
    tab = torch.from_numpy(addr.reshape(-1).view(np.int64)).cuda()
    assert tab.data_ptr() % 16 == 0
    return tab


def check_scattered(buf, index, values, what):
    """Every addressed float holds its parameter's value, every other float the sentinel, bit for bit."""
    h = buf.cpu()
    want = torch.full_like(h, SENT)
    rows, cols = np.nonzero(index >= 0)
    want[torch.from_numpy(index[rows, cols])] = values[torch.from_numpy(rows)]
    assert same(h, want), "%s: %d floats differ" % (what, int((bits(h) != bits(want)).sum()))


@pytest.mark.parametrize("slots", [2, 4])
@pytest.mark.parametrize("how", ["fused", "dp"])
def test_adam_scatter_tables(slots, how):
    """Hand-made tables at an n with a tail (both scatter paths run): empty slots, one slot, all slots."""
    c = O.adam_case(1023, 2, 8, 2, 1.0)
    base = run_adam(c, "fused")
    index, length = O.scatter_layout(c.n, slots)
    index_t, length_t = O.scatter_layout(c.n, slots, seed=11)
    assert (index[c.n - 3:] >= 0).any() and (index[:c.n - 3] >= 0).any()
    for with_target_table in (True, False):
        buf, buf_t = torch.full((length,), SENT).cuda(), torch.full((length_t,), SENT).cuda()
        tab, tab_t = table_for(index, buf), table_for(index_t, buf_t)
        run = run_adam(c, how, scatter=tab, scatter_target=tab_t if with_target_table else None, slots=slots)
        same_run(base, run, "the step with scatter tables against the step without")
        check_scattered(buf, index, run[0]["p"], "scatter (%d slots)" % slots)
        check_scattered(buf_t, index_t if with_target_table else np.full_like(index_t, -1), run[0]["target"],
                        "scatter_target (%d slots)" % slots)
    # a target table alone
    buf_t = torch.full((length_t,), SENT).cuda()
    run = run_adam(c, how, scatter_target=table_for(index_t, buf_t), slots=slots)
    same_run(base, run, "the step with a target table alone")
    check_scattered(buf_t, index_t, run[0]["target"], "scatter_target alone (%d slots)" % slots)


def test_adam_all_zero_and_overflowing_gradients():
    c = O.adam_case(1023, 2, 8, 2, 1.0)
    zero = torch.zeros(c.n)
    for how in ("fused", "split"):
        out, _ = run_adam(c, how, inputs=dict(c.inputs, m=zero, v=zero), grad=torch.zeros_like(c.grad))
        assert same(out["p"], c.inputs["p"]), "all-zero g, m, v moved p (%s)" % how
        assert same(out["m"], zero) and same(out["v"], zero)
        # g = 1e20: (f32(1 - 0.999) g) g = 1e37 does not overflow yet (optim_common.adam_big_gradient): an ordinary step
        _, grad, inputs = O.adam_big_gradient(1e20)
        out, st = run_adam(c, how, grad=grad)
        ss, bc = check_state(st, c.t)
        ref, bar = T.reference_and_bar("adam", lambda q: O.adam(q, ss, bc, O.TAU), inputs, k=1)
        assert bool(torch.isfinite(out["v"]).all()) and float(out["v"].min()) > 9e36
        hold([{k: (T.bar_ratio(out[k].numpy(), ref[k], O.K["adam_" + k] * bar[k]), "%s, every gradient entry 1e20" % how,
                   out[k], ref[k]) for k in out}])
        # g = 1e21: it overflows, v = +inf and the step is m / inf = 0 - the float32 formula's own result
        out, _ = run_adam(c, how, grad=O.adam_big_gradient(1e21)[1])
        assert bool(torch.isinf(out["v"]).all()) and bool((out["v"] > 0).all()), "v is not +inf at g = 1e21 (%s)" % how
        assert same(out["p"], c.inputs["p"]), "g = 1e21 moved p (%s)" % how
        assert bool(torch.isfinite(out["m"]).all()) and bool((out["m"] > 9e19).all())
        assert bool(torch.isfinite(out["target"]).all())


@pytest.mark.parametrize("bad", [NAN, float("inf")])
@pytest.mark.parametrize("where", ["body", "tail"])
def test_adam_one_non_finite_gradient_entry_stays_in_its_element(bad, where):
    """One NaN (or +inf) in one element of one slab: that element's p, m, v, target and scatter slots are non-finite,
    every other element - its three float4 neighbours included - is what it is without it, bit for bit."""
    c = O.adam_case(1023, 5, 8, 2, 1.0)
    e = 4 * 130 + 1 if where == "body" else c.n - 2
    index, length = O.scatter_layout(c.n, 2)
    index[e] = np.sort(np.setdiff1d(np.arange(length), index[index >= 0]))[:2]        # the element has both slots
    grad = c.grad.clone()
    grad[3, e] = bad
    runs = []
    for g in (c.grad, grad):
        buf, buf_t = torch.full((length,), SENT).cuda(), torch.full((length,), SENT).cuda()
        out, st = run_adam(c, "fused", grad=g, scatter=table_for(index, buf), scatter_target=table_for(index, buf_t))
        runs.append(dict(out, scat=buf.cpu(), scat_t=buf_t.cpu()))
        check_state(st, c.t)
    clean, dirty = runs
    others = torch.ones(c.n, dtype=torch.bool)
    others[e] = False
    for k in ("p", "m", "v", "target"):
        assert not bool(torch.isfinite(dirty[k][e])), "%s[%d] is finite: %r" % (k, e, float(dirty[k][e]))
        assert bool(torch.isfinite(clean[k]).all())
        assert same(dirty[k][others], clean[k][others]), "%s: the non-finite gradient entry reached another element" % k
    slots = torch.zeros(length, dtype=torch.bool)
    slots[torch.from_numpy(index[e])] = True
    for k in ("scat", "scat_t"):
        assert not bool(torch.isfinite(dirty[k][slots]).any()) and same(dirty[k][~slots], clean[k][~slots]), k


# ---------------------------------------------------------------------------
# temperature refresh and mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_mirror", O.MIRRORS)
def test_alpha_refresh_and_mirror(n_mirror):
    c = O.adam_case(O.ALPHA_N, 2, 8, 2, 1.0)
    base = run_adam(c, "fused")
    msrc_host = torch.randn(n_mirror, generator=T.gen(3 + n_mirror))
    worst = (0.0, "")
    for offs in O.ALPHA_OFFS:
        for inside in (True, False):
            for mirrored in (True, False):
                what = "offsets %s, dst %s the block, %s" % (offs, "inside" if inside else "outside",
                                                             "mirror %d" % n_mirror if mirrored else "no mirror")
                msrc, aout = guarded(msrc_host), guarded(torch.full((2,), NAN))
                mdst = torch.full((n_mirror + GUARD,), SENT).pin_memory()
                # where alpha k goes: float j of the mirrored block (distinct floats), or a float outside it
                slot = [(n_mirror - 1 - 5 * k) if inside and n_mirror - 1 - 5 * k >= 0 else None for k in range(len(offs))]
                dst = [aout.data_ptr() + 4 * k if j is None else msrc.data_ptr() + 4 * j for k, j in enumerate(slot)]
                run = run_adam(c, "fused", alpha=(offs, dst), mirror=(msrc.data_ptr(), mdst.data_ptr(), n_mirror) if mirrored else None)
                same_run(base, run, "the step with a temperature refresh against the step without (%s)" % what)
                src_after, out_after = unguard(msrc, n_mirror, "mirror_src"), unguard(aout, 2, "alpha_dst")
                want_src = msrc_host.clone()
                for k, j in enumerate(slot):
                    a = src_after[j] if j is not None else out_after[k]
                    ref, bar = O.exp_reference(run[0]["p"][offs[k]:offs[k] + 1].numpy())
                    r = O.np_ratio(np.array([float(a)]), ref, O.K["exp"] * bar)
                    print("device / bar  exp          %-60s %.3f" % (what, r))
                    worst = max(worst, (r, what))
                    if j is not None:
                        want_src[j] = a
                assert same(src_after, want_src), "the block changed outside the refreshed entries (%s)" % what
                for k in range(2):
                    if k >= len(offs) or slot[k] is not None:
                        assert bool(torch.isnan(out_after[k])), "a float no entry points at was written (%s)" % what
                # refreshed entries go out as the thread computed them, every other entry as mirror_src holds it
                want = torch.full_like(mdst, SENT)
                if mirrored:
                    want[:n_mirror] = want_src
                assert same(mdst, want), "mirror (%s): %d floats differ" % (what, int((bits(mdst) != bits(want)).sum()))
    assert worst[0] <= 1.0, "expf: %.3f of the bar (K = %d; %s)" % (worst[0], O.K["exp"], worst[1])


# ---------------------------------------------------------------------------
# streaming helpers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.STREAM_N)
def test_reduce_slabs_is_the_float32_sum_in_slab_order(n):
    for n_slabs in (1, 2, 9):
        for stride in (n, n + 5):
            grad = torch.full((n_slabs, stride), NAN)
            grad[:, :n] = torch.randn(n_slabs, n, generator=T.gen(n_slabs + stride % 1000)) * 10.0 ** torch.arange(n_slabs)[:, None]
            out = guarded(torch.full((n,), NAN))
            gr = guarded(grad.reshape(-1))
            call("nlbac_reduce_slabs", out.data_ptr(), gr.data_ptr(), n_slabs, stride, n)
            torch.cuda.synchronize()
            want = torch.from_numpy(O.reduce_slabs(grad.numpy(), n))
            assert same(unguard(out, n, "out"), want), "n %d, %d slabs %d apart" % (n, n_slabs, stride)


@pytest.mark.parametrize("n_cols", [1, 2, 4, 64, 65])
def test_sum_partials_sums_in_block_order_then_multiplies(n_cols):
    for n_blk in (1, 2, 300):
        for mul in (1.0, T.f32(1.0 / 7.0)):
            part = torch.randn(n_blk, n_cols, generator=T.gen(n_blk + n_cols)) * 3
            out = guarded(torch.full((n_cols,), NAN))
            pd = guarded(part.reshape(-1))
            call("nlbac_sum_partials", pd.data_ptr(), n_blk, n_cols, mul, out.data_ptr())
            torch.cuda.synchronize()
            want = torch.from_numpy(O.sum_partials(part.numpy(), mul))
            assert same(unguard(out, n_cols, "out"), want), "%d blocks of %d columns, mul %r" % (n_blk, n_cols, mul)


def test_fill_is_exact():
    for n in (1, 257, O.GRID + 77):
        for val in (-0.0, NAN, 1.5):
            buf = guarded(torch.full((n,), 7.0))
            call("nlbac_fill", buf.data_ptr(), val, n)
            torch.cuda.synchronize()
            assert same(unguard(buf, n, "fill"), torch.full((n,), val)), (n, val)


@pytest.mark.parametrize("block_len,n_blocks", [(1, 1), (1, 7), (6, 1), (6, 7), (1000, 1), (1000, 7), (1000, 530)])
def test_copy_blocks_moves_bits_between_strides(block_len, n_blocks):
    """Source and destination strides differ and exceed block_len; the gaps keep their sentinels.  The payload is int32
    bit patterns (NaN payloads, denormals): it moves bits."""
    assert (block_len, n_blocks) != (1000, 530) or block_len * n_blocks > O.GRID
    ss, ds = block_len + 3, block_len + 5
    rng = np.random.RandomState(block_len + n_blocks)
    words = rng.randint(-2 ** 31, 2 ** 31, size=(n_blocks, block_len), dtype=np.int64).astype(np.int32)
    words[0, 0] = 0x7FC12345                                   # a NaN with a payload
    src_bits = bits(torch.full((n_blocks, ss), SENT)).clone()
    src_bits[:, :block_len] = torch.from_numpy(words)
    src = src_bits.view(F32)
    dst = guarded(torch.full((n_blocks * ds,), SENT))
    sd = guarded(src.reshape(-1))
    call("nlbac_copy_blocks", sd.data_ptr(), ss, dst.data_ptr(), ds, block_len, n_blocks)
    torch.cuda.synchronize()
    got = unguard(dst, n_blocks * ds, "dst").reshape(n_blocks, ds)
    assert torch.equal(bits(got[:, :block_len]), torch.from_numpy(words))
    assert same(got[:, block_len:], torch.full((n_blocks, ds - block_len), SENT)), "the gaps between blocks were written"
    assert same(unguard(sd, n_blocks * ss, "src").reshape(n_blocks, ss), src), "the source changed"


def stream_compare(c, got, what=""):
    ref, bar = O.stream_reference(c.op, c.n, c.mag)
    k, = ref
    r = T.bar_ratio(got.numpy(), ref[k], O.K[c.op] * bar[k])
    print("device / bar  %-12s %-60s %.3f" % (c.op, c.label + what, r))
    assert r <= 1.0, "%s (%s): %.3f of the bar (K = %d)" % (c.op, c.label + what, r, O.K[c.op])
    vec_close(got.numpy(), ref[k].numpy(), 1e-4, "%s (%s)" % (c.op, c.label))


def test_axpby():
    for c in [c for c in O.stream_cases() if c.op == "axpby"]:
        x, y = guarded(c.inputs["x"]), guarded(c.inputs["y"])
        out = guarded(torch.full((c.n,), NAN))
        call("nlbac_axpby", c.a, x.data_ptr(), c.b, y.data_ptr(), c.n, out.data_ptr())
        torch.cuda.synchronize()
        stream_compare(c, unguard(out, c.n, "out"))
        assert same(unguard(x, c.n, "x"), c.inputs["x"]) and same(unguard(y, c.n, "y"), c.inputs["y"])
    # exact: a = b = 1 on integers below 2^20; y null with a = 1 and a = 0; in place
    for n in (1, 257, O.GRID + 77):
        g = T.gen(n % 1000)
        xi = torch.randint(-(1 << 19), 1 << 19, (n,), generator=g).float()
        yi = torch.randint(-(1 << 19), 1 << 19, (n,), generator=g).float()
        xr = torch.randn(n, generator=g)
        for a, x, b, y, want in ((1.0, xi, 1.0, yi, xi + yi), (1.0, xr, 5.0, None, xr), (0.0, xr, 5.0, None, torch.zeros(n)),
                                 (2.0, xi, -1.0, yi, 2 * xi - yi)):
            xd, yd = guarded(x), None if y is None else guarded(y)
            out = guarded(torch.full((n,), NAN))
            call("nlbac_axpby", a, xd.data_ptr(), b, ptr(yd), n, out.data_ptr())
            call("nlbac_axpby", a, xd.data_ptr(), b, ptr(yd), n, xd.data_ptr())          # in place: out == x
            torch.cuda.synchronize()
            assert same(unguard(out, n, "out"), want), "axpby a %g b %g n %d" % (a, b, n)
            assert same(unguard(xd, n, "x, in place"), want), "axpby in place a %g b %g n %d" % (a, b, n)


def test_soft_update():
    for c in [c for c in O.stream_cases() if c.op == "soft_update"]:
        tg, src = guarded(c.inputs["target"]), guarded(c.inputs["src"])
        call("nlbac_soft_update", tg.data_ptr(), src.data_ptr(), c.n, c.tau)
        torch.cuda.synchronize()
        stream_compare(c, unguard(tg, c.n, "target"))
        assert same(unguard(src, c.n, "src"), c.inputs["src"])
        for tau, want in ((0.0, c.inputs["target"]), (1.0, c.inputs["src"])):      # exact at both ends
            tg = guarded(c.inputs["target"])
            call("nlbac_soft_update", tg.data_ptr(), src.data_ptr(), c.n, tau)
            torch.cuda.synchronize()
            assert same(unguard(tg, c.n, "target"), want), "soft_update tau %g (%s)" % (tau, c.label)


@pytest.mark.parametrize("ld,n_rows", [(4, 1), (4, 255), (4, 257), (4, 600), (36, 1), (36, 28), (36, 29), (36, 67)])
def test_gather_rows_whole_rows_and_clamped_indices(ld, n_rows):
    """One lane per float4: n_rows ld / 4 = 1, 255, 257, 600 at ld 4, and 9, 252, 261, 603 at ld 36 (either side of a
    256-lane block).  Repeats, -5 (reads row 0) and src_rows + 3 (reads the last row)."""
    src_rows = 41
    src = O.sample_source(src_rows, ld)
    idx = torch.randint(0, src_rows, (n_rows,), generator=T.gen(ld + n_rows))
    idx[::7] = 3                                               # repeats
    if n_rows > 2:
        idx[1], idx[n_rows - 1] = -5, src_rows + 3
    else:
        idx[0] = src_rows + 3
    sd, idd = guarded(src.reshape(-1)), idx.cuda()
    dst = guarded(torch.full((n_rows * ld,), NAN))
    call("nlbac_gather_rows", sd.data_ptr(), src_rows, ld, idd.data_ptr(), n_rows, dst.data_ptr())
    torch.cuda.synchronize()
    assert same(unguard(dst, n_rows * ld, "dst").reshape(n_rows, ld), src[idx.clamp(0, src_rows - 1)])
    if n_rows == 1:
        dst = guarded(torch.full((ld,), NAN))
        call("nlbac_gather_rows", sd.data_ptr(), src_rows, ld, torch.tensor([-5]).cuda().data_ptr(), 1, dst.data_ptr())
        torch.cuda.synchronize()
        assert same(unguard(dst, ld, "dst"), src[0])


# ---------------------------------------------------------------------------
# the device draw
# ---------------------------------------------------------------------------
def sample_rows(src_dev, src_rows, ld, n_rows, n_eps, seed, draw, head=None, cap=None):
    """One nlbac_sample_rows (or, with ``head`` = the length the ring's head holds, nlbac_sample_rows_head) launch ->
    (rows (n_rows, ld), eps (n_eps) or None) on the host, guards checked."""
    dst = guarded(torch.full((n_rows * ld,), NAN))
    eps = guarded(torch.full((n_eps,), NAN)) if n_eps else None
    if head is None:
        call("nlbac_sample_rows", src_dev.data_ptr(), src_rows, ld, n_rows, dst.data_ptr(), ptr(eps), n_eps, seed, draw)
    else:
        for half in (0, 1):                                     # {position, length} twice: the other half is garbage
            hd = torch.full((2, 2), -77, dtype=torch.int64)
            hd[half, 0], hd[half, 1] = 5, head
            hd = hd.cuda()
            if half:
                dst = guarded(torch.full((n_rows * ld,), NAN))
                eps = guarded(torch.full((n_eps,), NAN)) if n_eps else None
            call("nlbac_sample_rows_head", src_dev.data_ptr(), hd.data_ptr(), half, cap, ld, n_rows, dst.data_ptr(),
                 ptr(eps), n_eps, seed, draw)
            torch.cuda.synchronize()
            assert hd.cpu()[half].tolist() == [5, head]
    torch.cuda.synchronize()
    return (unguard(dst, n_rows * ld, "dst").reshape(n_rows, ld), None if eps is None else unguard(eps, n_eps, "eps"))


def hold_noise(eps, seed, draw, what):
    ref, bar = O.noise_reference(seed, draw, len(eps))
    r = O.np_ratio(eps.numpy(), ref, O.K["noise"] * bar)
    assert bool(torch.isfinite(eps).all())
    return r, what


@pytest.mark.parametrize("pair", range(4))
def test_sample_rows_is_the_restated_draw(pair):
    """Rows: the restated index, whole rows, bit for bit.  Noise: inside the bar of the float64 formula; the float behind
    a ragged last quad is the sentinel (``unguard``)."""
    seed, draw = O.PAIRS[pair]
    ratios = []
    for src_rows in O.SAMPLE_SRC_ROWS:
        for ld in O.SAMPLE_LD:
            src = O.sample_source(src_rows, ld)
            sd = guarded(src.reshape(-1))
            for n_rows in O.SAMPLE_ROWS:
                idx = O.row_indices(seed, draw, n_rows, src_rows)
                for n_eps in O.sample_n_eps(n_rows, ld):
                    what = "seed %#x draw %#x: %d rows of %d from %d, %d noise" % (seed, draw, n_rows, ld, src_rows, n_eps)
                    rows, eps = sample_rows(sd, src_rows, ld, n_rows, n_eps, seed, draw)
                    assert np.array_equal(rows[:, 0].numpy().astype(np.int64), idx), "row indices (%s)" % what
                    assert same(rows, src[torch.from_numpy(idx)]), "rows (%s)" % what
                    if n_eps:
                        ratios.append(hold_noise(eps, seed, draw, what))
                    else:
                        assert eps is None
    for r, what in ratios:
        print("device / bar  noise        %-72s %.3f" % (what, r))
    for r, what in ratios:
        assert r <= 1.0, "noise (%s): %.3f of the bar (K = %d)" % (what, r, O.K["noise"])


def test_the_four_pairs_draw_four_different_minibatches():
    src = O.sample_source(3000, 4)
    sd = guarded(src.reshape(-1))
    got = [sample_rows(sd, 3000, 4, 300, 64, seed, draw) for seed, draw in O.PAIRS]
    for i in range(4):
        assert np.array_equal(got[i][0][:, 0].numpy().astype(np.int64), O.row_indices(*O.PAIRS[i], 300, 3000))
        for j in range(i):
            assert not same(got[i][0], got[j][0]) and not same(got[i][1], got[j][1]), (i, j)


@pytest.mark.parametrize("pair", range(4))
def test_sample_rows_head_is_sample_rows_at_the_heads_length(pair):
    seed, draw = O.PAIRS[pair]
    cap, ld, n_rows, n_eps = 3000, 36, 300, 301
    src = O.sample_source(cap, ld)
    sd = guarded(src.reshape(-1))
    for length in (1, 2, 1234, cap):
        want = sample_rows(sd, length, ld, n_rows, n_eps, seed, draw)
        got = sample_rows(sd, None, ld, n_rows, n_eps, seed, draw, head=length, cap=cap)
        assert same(got[0], want[0]) and same(got[1], want[1]), "a head length of %d" % length
        assert np.array_equal(got[0][:, 0].numpy().astype(np.int64), O.row_indices(seed, draw, n_rows, length))
    at_cap = sample_rows(sd, cap, ld, n_rows, n_eps, seed, draw)
    for length in (cap + 1, 1 << 40):                          # above cap: read as cap
        got = sample_rows(sd, None, ld, n_rows, n_eps, seed, draw, head=length, cap=cap)
        assert same(got[0], at_cap[0]) and same(got[1], at_cap[1]), "a head length of %d" % length
    for length in (0, -3):                                     # nothing is copied; the noise is still drawn
        got = sample_rows(sd, None, ld, n_rows, n_eps, seed, draw, head=length, cap=cap)
        assert bool(torch.isnan(got[0]).all()), "a head length of %d wrote rows" % length
        assert same(got[1], at_cap[1])


@pytest.mark.parametrize("pair", range(4))
def test_sample_windows_start_rows_are_the_restated_indices(pair):
    """The start rows of nlbac_sample_windows are the rows nlbac_sample_rows draws at equal (seed, draw, src_rows); the
    row number is planted in column 0."""
    seed, draw = O.PAIRS[pair]
    src_rows, cap, ld = 3000, 4096, 36
    src = torch.full((cap, ld), NAN)
    src[:src_rows] = O.sample_source(src_rows, ld)
    sd = guarded(src.reshape(-1))
    plain = guarded(O.sample_source(src_rows, ld).reshape(-1))
    for n in (300, 1):
        idx = O.row_indices(seed, draw, n, src_rows)
        rows, _ = sample_rows(plain, src_rows, ld, n, 0, seed, draw)
        assert np.array_equal(rows[:, 0].numpy().astype(np.int64), idx)
        for H in (1, 3):
            n_blk = (n + 255) // 256
            dst, valid = guarded(torch.full((H * n * ld,), NAN)), guarded(torch.full((n,), NAN))
            counts = torch.full((n_blk + GUARD,), STATE_GUARD, dtype=torch.int32).cuda()
            call("nlbac_sample_windows", sd.data_ptr(), src_rows, cap, src_rows, ld, n, H, 1, 4, 12, 3, dst.data_ptr(),
                 valid.data_ptr(), counts.data_ptr(), seed, draw)
            torch.cuda.synchronize()
            out = unguard(dst, H * n * ld, "dst").reshape(H, n, ld)
            assert np.array_equal(out[0, :, 0].numpy().astype(np.int64), idx), "start rows (n %d, H %d)" % (n, H)
            for k in range(H):      # step k: the row k pushes on, held at the newest row
                assert same(out[k], src[torch.from_numpy(np.minimum(idx + k, src_rows - 1))]), "step %d (n %d, H %d)" % (k, n, H)
            v, cnt = unguard(valid, n, "valid"), counts.cpu()
            assert bool((cnt[n_blk:] == STATE_GUARD).all())
            # H = 1: every window is valid; H = 3: the random rows are no episode, so none is
            assert same(v, torch.full((n,), 1.0 if H == 1 else 0.0))
            assert cnt[:n_blk].tolist() == [int(v[b * 256:(b + 1) * 256].sum()) for b in range(n_blk)]
