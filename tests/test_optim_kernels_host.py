"""The references, cases and bars of ``optim_common`` are themselves checked, on the CPU: the float32 evaluation of every
reference stays within half its bar on every case (the condition that fixes ``K``); the numpy restatement of the
device draw (``u01`` at its extreme words, the row index at the largest word, the four (seed, draw) pairs); and every
refusal of ``nlbac_adam_fused``, ``nlbac_adam_step`` and ``nlbac_gather_rows`` (no GPU needed: every pointer handed
over is host memory that a refused call never touches, and a refused call launches nothing)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import optim_common as O
import task_kernels_common as T
from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)

F32 = T.F32


# ---------------------------------------------------------------------------
# K
# ---------------------------------------------------------------------------
def test_float32_reference_within_half_the_bar():
    """The condition that fixes K: on every case the float32 evaluation of the reference is within half the bar, and no
    smaller power of two would do."""
    worst = {}

    def note(op, r, label):
        if r >= worst.get(op, (-1.0, ""))[0]:
            worst[op] = (r, label)

    for c in O.adam_cases():
        consts = O.step_consts(O.LR, c.t)
        ref, bar = O.adam_reference(c.key, *consts, O.TAU)
        lo = O.adam_float32(c.key, *consts, O.TAU)
        assert set(lo) == set(ref) == {"p", "m", "v", "target"}
        for k in ref:
            note("adam_" + k, T.bar_ratio(lo[k].double().numpy(), ref[k], O.K["adam_" + k] * bar[k]), c.label)
    c, _, inputs = O.adam_big_gradient(1e20)
    fn = lambda t: O.adam(t, *O.step_consts(O.LR, c.t), O.TAU)
    ref, bar = T.reference_and_bar("adam", fn, inputs, k=1)
    lo = T.run(fn, inputs, F32)
    assert bool(np.isfinite(lo["v"].numpy()).all()) and float(lo["v"].min()) > 9e36
    assert bool(np.isinf(T.run(fn, O.adam_big_gradient(1e21)[2], F32)["v"].numpy()).all())
    for k in ref:
        note("adam_" + k, T.bar_ratio(lo[k].double().numpy(), ref[k], O.K["adam_" + k] * bar[k]), "every gradient entry 1e20")
    for c in O.stream_cases():
        ref, bar = T.reference_and_bar(c.op, c.fn, c.inputs, k=O.K[c.op])
        lo = T.run(c.fn, c.inputs, F32)
        for k in ref:
            note(c.op, T.bar_ratio(lo[k].double().numpy(), ref[k], bar[k]), c.label)
    p = (np.random.RandomState(0).randn(4096) * 3).astype(np.float32)
    ref, bar = O.exp_reference(p)
    note("exp", O.np_ratio(np.exp(p), ref, O.K["exp"] * bar), "4096 draws of 3 N(0, 1)")
    seed, draw = O.PAIRS[0]
    ref, bar = O.noise_reference(seed, draw, 4 * 4096)
    note("noise", O.np_ratio(O.noise_float32(seed, draw, 4 * 4096), ref, O.K["noise"] * bar), "4096 quads")
    assert set(worst) == set(O.K)
    for op in O.K:
        print("float32 reference / bar  %-12s K %-3d %.3f   (%s)" % (op, O.K[op], worst[op][0], worst[op][1]))
    for op in O.K:
        assert worst[op][0] <= 0.5, "%s: the float32 reference is at %.3f of the bar (%s)" % ((op,) + worst[op])
        assert O.K[op] == 1 or worst[op][0] > 0.25, "%s: K = %d is not the smallest power of two" % (op, O.K[op])


def test_adam_cases_are_what_they_claim():
    cs = O.adam_cases()
    seen = {(c.n, c.n_slabs, c.stride - O.round4(c.n)) for c in cs}
    assert seen >= {(n, s, pad) for n in O.ADAM_N for s in O.ADAM_SLABS for pad in O.ADAM_PADS}
    assert {(c.t, c.mag) for c in cs} >= {(t, mag) for t in O.ADAM_STEPS for mag in O.ADAM_MAGS}
    assert O.ADAM_BIG_N > 2048 * 256 * 4 and O.ADAM_BIG_N % 4 == 3 and O.GRID + 77 > 2048 * 256
    for c in cs:
        assert c.stride % 4 == 0 and c.stride >= c.n
        assert bool(np.isnan(c.grad[:, c.n:].numpy()).all()) and bool(np.isfinite(c.grad[:, :c.n].numpy()).all())
        if c.t == 1:
            assert not c.inputs["m"].any() and not c.inputs["v"].any()
        else:
            assert bool((c.inputs["v"] > 0).all()) and bool((c.inputs["m"] != 0).all())
        if c.key[-1]:       # cancelling: the sum is a thousandth of a slab
            s = (c.inputs["g0"].double() + c.inputs["g1"].double()).abs().max()
            assert float(s) < 1e-2 * float(c.inputs["g0"].abs().max())
    for t in O.ADAM_STEPS:   # the constants are the float32 roundings the issue names
        ss, bc = O.step_consts(O.LR, t)
        assert ss == float(np.float32(O.LR / (1 - 0.9 ** t))) and bc == float(np.float32((1 - 0.999 ** t) ** 0.5))
    assert O.step_consts(O.LR, 10 ** 6) == (T.f32(O.LR), 1.0)


@pytest.mark.parametrize("slots", [2, 4])
def test_scatter_layout(slots):
    index, length = O.scatter_layout(1023, slots)
    used = index[index >= 0]
    assert len(np.unique(used)) == len(used) and used.max() < length and len(used) < length     # distinct; some float unaddressed
    assert abs((index < 0).mean() - 1 / 3) < 0.1                                                  # about a third: no slot
    per = (index >= 0).sum(1)
    assert set(per.tolist()) >= {0, 1, slots}
    assert bool((index[per == 1] >= 0).any(0).all())          # a lone slot stands at every position of an entry
    assert not np.array_equal(used, np.sort(used))            # shuffled


# ---------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------
def test_u01_is_exact_and_reaches_one():
    for x in O.U01_WORDS:
        exact = Fraction(x >> 8, 2 ** 24) + Fraction(1, 2 ** 25)
        got = O.u01(x)
        assert got.dtype == np.float32 and float(got) == float(np.float32(float(exact))), hex(x)   # (float(exact) is exact)
        assert 0.0 < float(got) <= 1.0
    vals = [float(O.u01(x)) for x in O.U01_WORDS]
    assert vals == [2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25, 0xFFFFFF * 2.0 ** -25, 1.0, 1.0]
    assert Fraction(0xFFFFFF, 2 ** 24) + Fraction(1, 2 ** 25) == 1 - Fraction(1, 2 ** 25)          # the tie below 1.0


def test_noise_is_finite_at_the_extreme_words():
    w = np.array(O.U01_WORDS, dtype=np.uint32)
    a, b = [v.reshape(-1) for v in np.meshgrid(w, w)]
    for dtype in (np.float32, np.float64):
        eps, bar = O.noise_from_words((a, b, b, a), dtype)
        assert eps.dtype == dtype and bool(np.isfinite(eps).all()) and bool(np.isfinite(bar).all())
        one = np.repeat(O.u01(a) == 1.0, 2)                   # u01 == 1: the radius is 0 and so is the noise
        assert one.any() and not eps.reshape(-1, 4)[:, :2].reshape(-1)[one].any()


def test_row_index_stays_inside_the_source():
    for src_rows in (1, 2, 3000, 2 ** 32 - 1):
        assert O.row_of(0xFFFFFFFF, src_rows) == src_rows - 1 < src_rows
        assert O.row_of(0, src_rows) == 0
    assert O.row_of(0x80000000, 3000) == 1500


def test_every_half_of_seed_and_draw_enters_the_draw():
    idx = [O.row_indices(seed, draw, 300, 3000) for seed, draw in O.PAIRS]
    eps = [O.noise_float32(seed, draw, 64) for seed, draw in O.PAIRS]
    for i in range(4):
        assert idx[i].min() >= 0 and idx[i].max() < 3000
        for j in range(i):
            assert not np.array_equal(idx[i], idx[j]) and not np.array_equal(eps[i], eps[j])
    # tag 0 and tag 1 are different streams, and the index is the FIRST word
    w = O.draw_words(5, 1, 8, 0)
    assert not np.array_equal(w[0], O.draw_words(5, 1, 8, 1)[0]) and not np.array_equal(w[0], w[1])
    assert O.row_indices(5, 1, 8, 3000).tolist() == [(int(x) * 3000) >> 32 for x in w[0]]


def test_noise_statistics():
    """65536 values of N(0, 1): five standard errors of the mean and of the std."""
    eps, _ = O.noise_reference(7, 3, 65536)
    assert abs(float(eps.mean())) <= 5 / 256 and abs(float(eps.std()) - 1) <= 5 / 362


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def host_block():
    """A 16-byte aligned address inside host memory that stands in for every device buffer."""
    host = (C.c_float * 96)()
    return (C.addressof(host) + 15) & ~15, host


def fused_args():
    """The arguments of an ``nlbac_adam_fused`` call that would be launched, by name and in the entry point's order."""
    from nlbac_amd import _lib
    p, host = host_block()
    kw = dict(p=p, m=p, v=p, grad=p, n_slabs=1, slab_stride=8, n=8, state=p, lr=O.LR, target=p, tau=0.005, scatter=None,
              scatter_target=None, scatter_slots=2, n_alpha=0, alpha_off=None, alpha_dst=None, mirror_src=None,
              mirror_dst=None, n_mirror=0, s=None)
    assert len(kw) == len(_lib._PROTOS["nlbac_adam_fused"])
    return kw, p, host


def test_adam_fused_refuses_before_launching(lib):
    name = "nlbac_adam_fused"
    kw, p, keep = fused_args()
    off, dst = (C.c_long * 2)(3, 5), (C.c_void_p * 2)(p, p)
    assert "2 or 4" in refused(lib, name, dict(kw, scatter=p, scatter_slots=3), "scatter_slots = 3 with a table")
    assert "2 or 4" in refused(lib, name, dict(kw, scatter_target=p, scatter_slots=3), "scatter_slots = 3 with a target table")
    assert "scatter_target" in refused(lib, name, dict(kw, scatter_target=p, tau=-1.0), "scatter_target with tau < 0")
    assert "scatter_target" in refused(lib, name, dict(kw, scatter_target=p, target=None), "scatter_target without a target")
    for slots in (2, 4):       # two slots per 16-byte load: a table at 16 k + 8 is refused
        assert "aligned" in refused(lib, name, dict(kw, scatter=p + 8, scatter_slots=slots), "a table at 16 k + 8")
        assert "aligned" in refused(lib, name, dict(kw, scatter=p, scatter_target=p + 8, scatter_slots=slots),
                                    "a target table at 16 k + 8")
    assert "alpha" in refused(lib, name, dict(kw, n_alpha=3, alpha_off=off, alpha_dst=dst), "n_alpha = 3")
    assert "alpha" in refused(lib, name, dict(kw, n_alpha=-1, alpha_off=off, alpha_dst=dst), "n_alpha = -1")
    assert "alpha" in refused(lib, name, dict(kw, n_alpha=1), "n_alpha = 1 without the arrays")
    for bad in ((8, 0), (3, 8), (-1, 0), (1 << 40, 0)):
        n_alpha = 2 if bad[0] == 3 else 1
        assert "out of range" in refused(lib, name, dict(kw, n_alpha=n_alpha, alpha_off=(C.c_long * 2)(*bad), alpha_dst=dst),
                                         "alpha offsets %s with n = 8" % (bad,))
    assert "out of range" in refused(lib, name, dict(kw, n_alpha=1, alpha_off=off, alpha_dst=(C.c_void_p * 2)(None, p)),
                                     "a null alpha destination")
    for n_mirror in (0, 1025, -1):
        assert "mirror" in refused(lib, name, dict(kw, mirror_src=p, mirror_dst=p, n_mirror=n_mirror),
                                   "n_mirror = %d with a mirror" % n_mirror)
    assert "mirror" in refused(lib, name, dict(kw, mirror_dst=p, n_mirror=4), "a mirror without a source")
    assert "sizes" in refused(lib, name, dict(kw, lr=0.0), "lr = 0")
    assert "sizes" in refused(lib, name, dict(kw, lr=-1e-3), "lr < 0")
    assert "sizes" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "sizes" in refused(lib, name, dict(kw, n_slabs=0), "n_slabs = 0")
    for stride in (6, 9, 10, 11):
        assert "aligned" in refused(lib, name, dict(kw, slab_stride=stride), "slab_stride = %d" % stride)
    for k in ("p", "m", "v", "grad", "target"):
        assert "aligned" in refused(lib, name, dict(kw, **{k: p + 4}), "%s at 16 k + 4" % k)
    for k in ("p", "m", "v", "grad", "state"):
        assert "null" in refused(lib, name, dict(kw, **{k: None}), "a null %s" % k)


def test_adam_step_refuses_before_launching(lib):
    from nlbac_amd import _lib
    name = "nlbac_adam_step"
    p, keep = host_block()
    kw = dict(p=p, m=p, v=p, grad=p, n_slabs=1, slab_stride=8, n=8, state=p, target=p, tau=0.005, s=None)
    assert len(kw) == len(_lib._PROTOS[name])
    assert "aligned" in refused(lib, name, dict(kw, slab_stride=6), "slab_stride = 6")
    for k in ("p", "m", "v", "grad", "target"):
        assert "aligned" in refused(lib, name, dict(kw, **{k: p + 4}), "%s at 16 k + 4" % k)
    for k in ("p", "m", "v", "grad", "state"):
        assert "null" in refused(lib, name, dict(kw, **{k: None}), "a null %s" % k)
    assert "sizes" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "null" in refused(lib, "nlbac_adam_prepare", dict(state=None, lr=O.LR, s=None), "a null state")


def test_gather_and_sample_rows_refuse_before_launching(lib):
    p, keep = host_block()
    kw = dict(src=p, src_rows=5, ld=4, idx=p, n_rows=3, dst=p, s=None)
    for ld in (6, 0, 2, -4):
        assert "float4" in refused(lib, "nlbac_gather_rows", dict(kw, ld=ld), "ld = %d" % ld)
    assert "float4" in refused(lib, "nlbac_gather_rows", dict(kw, dst=p + 4), "dst at 16 k + 4")
    assert "bad arguments" in refused(lib, "nlbac_gather_rows", dict(kw, src_rows=0), "src_rows = 0")
    kw = dict(src=p, src_rows=5, ld=4, n_rows=3, dst=p, eps=p, n_eps=4, seed=1, draw=1, s=None)
    assert "float4" in refused(lib, "nlbac_sample_rows", dict(kw, ld=6), "ld = 6")
    assert "bad arguments" in refused(lib, "nlbac_sample_rows", dict(kw, src_rows=1 << 32), "src_rows = 2^32")
    assert "bad arguments" in refused(lib, "nlbac_sample_rows", dict(kw, src_rows=0), "src_rows = 0")
    assert "n_eps" in refused(lib, "nlbac_sample_rows", dict(kw, eps=None), "n_eps without a buffer")


def test_header_states_the_table_alignment():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    doc = header[header.index("nlbac_adam_prepare + nlbac_adam_step + nlbac_mlp_pack"):header.index("int nlbac_adam_fused(")]
    assert "16-byte aligned" in doc and "refused" in doc
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in header
    assert "// (0, 1]" in open(os.path.join(_lib.CSRC, "philox.h")).read()      # u01's range, as the host test above finds it
