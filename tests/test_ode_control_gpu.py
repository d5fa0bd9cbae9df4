"""The dopri5 step control and the per-row RK glue (``csrc/ode_kernels.hip`` through ``nlbac_dopri_interp_bwd``,
``csrc/ode_control.h``, the per-row glue of ``csrc/node_adjoint_kernels.hip``), each entry point launched on its own
through the C ABI and held to the float64 references and bars of ``ode_control_common`` (``K`` fixed on the CPU, see
there) and to ``vec_close(..., 1e-4)``; the controller's doubles are held to 1e-12 and copies to exact equality.  Every
output has NaN prefill and a guard row (partials, control blocks, step slots: a guard block) of sentinels, and a leading
dimension wider than the logical width where the ABI has one.  Each check prints its device / bar ratio before it
asserts.  No MFMA kernel is launched and no solve is run."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ode_control_common as Q
import task_kernels_common as T
from common import vec_close

pytestmark = pytest.mark.gpu
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
SENT = T.SENTINEL


def lib():
    from nlbac_amd import _lib
    return _lib


def stream():
    from nlbac_amd.arena import stream_ptr
    return stream_ptr()


def call(name, *args):
    lib().call(name, *(args + (stream(),)))


def dev(t):
    return t.contiguous().cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def fptr(vals):
    return lib().fptr(*[float(v) for v in vals])


def out_buf(rows, ld=1, fill=None, dtype=F32):
    """(rows + 1, ld) on the device: NaN (or ``fill`` (rows, ld)) with a guard row of sentinels."""
    buf = torch.full((rows + 1, ld), NAN, dtype=dtype)
    if fill is not None:
        buf[:rows] = torch.as_tensor(fill, dtype=dtype).reshape(rows, ld)
    buf[rows] = SENT
    return dev(buf)


def read(buf, rows, width, what):
    """The (rows, width) the kernel owns, after checking that it wrote nothing else: guard row and padding untouched."""
    h = buf.cpu()
    assert bool((h[rows] == SENT).all()), "%s: the guard row was written" % what
    assert bool(torch.isnan(h[:rows, width:]).all()), "%s: the padding columns were written" % what
    return h[:rows, :width]


# The interpolant's backward hands out ONE gradient, with respect to v = (y0, y1, K): vec_close takes it as one vector.
# At x = 1 its y0 part is identically zero (y(t0 + h) = y1 whatever y0 is) while the kernel is left with the rounding of
# (1 - 8 + 18 - 11) g, so that part has no scale of its own.
ONE_VECTOR = ("interp_bwd", "interp_map_bwd")


def compare(c, got, what=""):
    """Every tensor of ``got`` against the float64 reference of case ``c``: bar, then vec_close 1e-4."""
    ref, bar = Q.reference_and_bar(c.op, c.fn, c.inputs)
    return compare_ref(c.op, ref, bar, got, c.label + what)


def compare_ref(op, ref, bar, got, what):
    ratios = {k: Q.bar_ratio(x.numpy(), ref[k], bar[k]) for k, x in got.items()}
    for k, r in ratios.items():
        print("device / bar  %-16s %-9s %-52s %.3f" % (op, k, what, r))
    for k, r in ratios.items():
        assert r <= 1.0, "%s %s (%s): %.3f of the bar (K = %d)" % (op, k, what, r, Q.K[op])
        if op not in ONE_VECTOR:
            vec_close(got[k].numpy(), ref[k].numpy(), 1e-4, "%s %s (%s)" % (op, k, what))
    if op in ONE_VECTOR:
        flat = lambda d: np.concatenate([d[k].numpy().reshape(-1) for k in sorted(got)])
        vec_close(flat(got), flat(ref), 1e-4, "%s (%s)" % (op, what))
    return ref, bar


def h_block(h):
    """The steps as a launch reads them from control blocks: (P, 16) doubles, C_H set and the rest NaN."""
    c = torch.full((len(h), Q.CTL), NAN, dtype=F64)
    c[:, Q.C_H] = torch.tensor(h, dtype=F64)
    return dev(c)


def by_rows(cases, rows):
    return [c for c in cases if (c.meta.key[0] if hasattr(c.meta, "key") else c.meta.n) == rows]


# ---------------------------------------------------------------------------
# RK algebra
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", Q.ROWS)
def test_affine_combine(n):
    for c in by_rows(Q.affine_cases(), n):
        m, t = c.meta, c.inputs
        g, u = dev(t["g"]), dev(t["u"])
        if c.op == "affine_fwd":
            k, f = out_buf(n, m.n_s), dev(t["f"])
            call("nlbac_affine_combine_fwd", f.data_ptr(), g.data_ptr(), u.data_ptr(), m.n_s, m.n_u, n, k.data_ptr())
            torch.cuda.synchronize()
            compare(c, dict(k=read(k, n, m.n_s, "k")))
            continue
        dg = out_buf(n, m.n_s * m.n_u) if m.want_dg else None
        du = None if m.du_mode == "null" else out_buf(n, m.n_u, t.get("du0"))
        dk = dev(t["dk"])
        call("nlbac_affine_combine_bwd", dk.data_ptr(), g.data_ptr(), u.data_ptr(), m.n_s, m.n_u, n, m.mul,
             ptr(dg), ptr(du), int(m.du_mode == "accumulate"))
        torch.cuda.synchronize()
        got = {}
        if dg is not None:
            got["dg"] = read(dg, n, m.n_s * m.n_u, "dg").reshape(n, m.n_s, m.n_u)
        if du is not None:
            got["du"] = read(du, n, m.n_u, "du")
        compare(c, got)


@pytest.mark.parametrize("rows", Q.ROWS)
def test_rk_combine(rows):
    for c in by_rows(Q.rk_combine_cases(), rows):
        m, t = c.meta, c.inputs
        s = Q.state_case(*m.key)
        Kd = dev(t["K"])
        hd = h_block(s.h) if m.h_dev else None
        out = out_buf(s.n, s.n_s)
        y0 = dev(t["y0"]) if m.y0 else None
        call("nlbac_rk_combine", ptr(y0), Kd.data_ptr(), len(m.coef), fptr(m.coef),
             None if m.h_dev else fptr(s.h), ptr(hd), Q.CTL if m.h_dev else 0, s.P, s.rows, s.n_s, out.data_ptr())
        torch.cuda.synchronize()
        got = read(out, s.n, s.n_s, "out")
        assert bool(torch.isfinite(got).all()), "a stage behind a zero coefficient was read"
        compare(c, dict(out=got))


def test_rk_combine_without_stages():
    s = Q.state_case(257, 3, 6, 2)
    y0, Kd = dev(s.y0), dev(s.K)
    for with_y0 in (True, False):
        out = out_buf(s.n, s.n_s)
        call("nlbac_rk_combine", y0.data_ptr() if with_y0 else None, Kd.data_ptr(), 0, fptr([0.0]), fptr(s.h), None, 0,
             s.P, s.rows, s.n_s, out.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(read(out, s.n, s.n_s, "out"), s.y0 if with_y0 else torch.zeros_like(s.y0))


@pytest.mark.parametrize("rows", Q.ROWS)
def test_rk_stage_bwd(rows):
    for c in by_rows(Q.rk_stage_bwd_cases(), rows):
        m, t = c.meta, c.inputs
        s = Q.state_case(*m.key)
        d = {k: dev(t[k]) for k in m.srcs}
        dK = out_buf(4 * s.n, s.n_s, t["dK0"])
        dy0 = None if m.dy0_mode == "null" else out_buf(s.n, s.n_s, t.get("dy0_0"))
        du = out_buf(s.n, m.n_ext, t["du_ext0"]) if m.n_ext else None
        hd = h_block(s.h) if m.h_dev else None
        call("nlbac_rk_stage_bwd", ptr(d.get("dYup")), ptr(d.get("dXf")), ptr(d.get("dXg")), m.ld, 4, fptr(Q.COEF4),
             None if m.h_dev else fptr(s.h), ptr(hd), Q.CTL if m.h_dev else 0, s.P, s.rows, s.n_s, dK.data_ptr(), ptr(dy0),
             int(m.dy0_mode == "accumulate"), ptr(du), m.n_ext)
        torch.cuda.synchronize()
        stages = read(dK, 4 * s.n, s.n_s, "dK").reshape(4, s.n, s.n_s)
        assert bool(torch.isnan(stages[2]).all()), "the stage behind the zero coefficient was written"
        got = dict(dK=stages[Q.live(Q.COEF4)])
        if dy0 is not None:
            got["dy0"] = read(dy0, s.n, s.n_s, "dy0")
        if du is not None:
            got["du_ext"] = read(du, s.n, m.n_ext, "du_ext")
        compare(c, got)


# ---------------------------------------------------------------------------
# norm sums
# ---------------------------------------------------------------------------
def nblk_of(rpp):
    return -(-rpp // Q.BLOCK)


def norm_args(t, n_u):
    """(a, b, y0, y1, u) device tensors of a ``norm_sums`` input dict (u: a dummy where the case has no action columns)."""
    d = {k: dev(v) for k, v in t.items()}
    if "u" in d and n_u == 0:
        d["u"] = dev(torch.zeros(1))
    return d, (ptr(d.get("a")), ptr(d.get("b")), ptr(d.get("y0")), ptr(d.get("y1")), ptr(d.get("u")))


@pytest.mark.parametrize("rows", Q.ROWS)
def test_dopri_norm_partials(rows):
    for c in by_rows(Q.norm_cases(), rows):
        s = Q.state_case(*c.meta.key)
        nb = nblk_of(s.rows)
        keep, args = norm_args(c.inputs, s.n_u)
        part = out_buf(s.P * nb, 2)
        call("nlbac_dopri_norm_partials", *args, c.meta.mode, s.rtol, s.atol, s.n_s, s.n_u, s.rows, s.P, part.data_ptr(),
             None, 0)
        torch.cuda.synchronize()
        compare(c, dict(partials=read(part, s.P * nb, 2, "partials").reshape(s.P, nb, 2)))


@pytest.mark.parametrize("row", [0, 255, 256, 599])
def test_dopri_norm_partials_one_hot(row):
    """One non-zero row in the second of three problems: its block holds the value, every other block is exactly 0."""
    rpp, P, n_s, n_u, nb = 600, 3, 6, 2, 3
    g = T.gen(50 + row)
    hot = rpp + row
    y0, y1 = T.randn(g, P * rpp, n_s), T.randn(g, P * rpp, n_s)
    for mode in (0, 2):
        a = torch.zeros(P * rpp, n_s)
        a[hot] = T.randn(g, n_s) * 1e-5
        if mode == 0:
            t = dict(y0=torch.zeros(P * rpp, n_s), a=a, u=torch.zeros(P * rpp, n_u))
            t["y0"][hot] = T.randn(g, n_s)
        else:
            t = dict(y0=y0, y1=y1, a=a)
        keep, args = norm_args(t, n_u)
        part = out_buf(P * nb, 2)
        call("nlbac_dopri_norm_partials", *args, mode, 1e-5, 1e-7, n_s, n_u, rpp, P, part.data_ptr(), None, 0)
        torch.cuda.synchronize()
        got = read(part, P * nb, 2, "partials").reshape(P, nb, 2)
        op = "norm_sums%d" % mode
        fn = lambda q: Q.norm_sums(mode, q, 1e-5, 1e-7, rpp, P)
        ref, bar = Q.reference_and_bar(op, fn, t)
        compare_ref(op, ref, bar, dict(partials=got), "one-hot row %d" % row)
        mask = torch.ones(P, nb, 2, dtype=torch.bool)
        mask[1, row // Q.BLOCK, :] = False
        assert bool((got[mask] == 0).all()) and bool((got[1, row // Q.BLOCK, 0] > 0))


def slot_buffers(s, slots, n_slots, extra=None):
    """The step-slot form of a shared case: err and y1 as (n_slots, n, n_s) with problem p's rows in slot ``slots[p]``
    and its y0 rows as the y1 of slot ``slots[p] - 1`` (slot 0: the caller's y0); everything else NaN."""
    E = torch.full((n_slots, s.n, s.n_s), NAN)
    Y1 = torch.full((n_slots, s.n, s.n_s), NAN)
    y0 = torch.full((s.n, s.n_s), NAN)
    for p, k in enumerate(slots):
        r = slice(p * s.rows, (p + 1) * s.rows)
        E[k, r], Y1[k, r] = s.err[r], s.y1[r]
        if k == 0:
            y0[r] = s.y0[r]
        else:
            Y1[k - 1, r] = s.y0[r]
    return dev(E), dev(Y1), dev(y0)


def test_dopri_norm_partials_step_slots():
    """Mode 2 with ``slot_ctl``: problem 0 works in slot 0 on the caller's y0, problem 1 in slot 2 on slot 1's y1, problem
    2 is done and its partials stay NaN."""
    key = (257, 3, 6, 2, 0)
    s = Q.state_case(*key)
    nb = nblk_of(s.rows)
    E, Y1, y0 = slot_buffers(s, (0, 2, 1), 3)
    ctl = torch.tensor([Q.ctl_block(p, nacc=k, done=float(p == 2)) for p, k in enumerate((0, 2, 1))], dtype=F64)
    d_ctl = dev(ctl)
    part = out_buf(s.P * nb, 2)
    call("nlbac_dopri_norm_partials", E.data_ptr(), None, y0.data_ptr(), Y1.data_ptr(), None, 2, s.rtol, s.atol, s.n_s,
         s.n_u, s.rows, s.P, part.data_ptr(), d_ctl.data_ptr(), s.n * s.n_s)
    torch.cuda.synchronize()
    got = read(part, s.P * nb, 2, "partials").reshape(s.P, nb, 2)
    assert bool(torch.isnan(got[2]).all()), "a finished problem's partials were written"
    c = [c for c in Q.norm_cases() if c.meta.key == key and c.meta.mode == 2][0]
    ref, bar = Q.reference_and_bar(c.op, c.fn, c.inputs)
    compare_ref(c.op, {"partials": ref["partials"][:2]}, {"partials": bar["partials"][:2]}, dict(partials=got[:2]),
                "step slots")
    assert torch.equal(d_ctl.cpu(), ctl)


@pytest.mark.parametrize("rows", Q.ROWS)
def test_adj_norm_sums_two_call_form(rows):
    """``nlbac_adj_norm_control`` without tickets writes the four sums and leaves the control block alone."""
    for c in by_rows(Q.adj_norm_cases(), rows):
        s = Q.adj_case(*c.meta.key)
        nb = nblk_of(s.rows)
        t = c.inputs
        d = {k: dev(v) for k, v in t.items()}
        if "u" in d and s.n_u == 0:
            d["u"] = dev(torch.zeros(1))
        ctl = torch.tensor([Q.ctl_block(p) for p in range(s.P)], dtype=F64)
        d_ctl = dev(ctl)
        part = out_buf(s.P * nb, 4)
        call("nlbac_adj_norm_control", ptr(d.get("a")), ptr(d.get("b")), ptr(d.get("Z0")), ptr(d.get("Z1")), ptr(d.get("u")),
             c.meta.mode, s.rtol, s.atol, s.n_s, s.n_u, s.rows, s.P, 1.0, None, part.data_ptr(), None, d_ctl.data_ptr(),
             None, 0.0)
        torch.cuda.synchronize()
        compare(c, dict(partials=read(part, s.P * nb, 4, "partials").reshape(s.P, nb, 4)))
        assert torch.equal(d_ctl.cpu(), ctl)


# ---------------------------------------------------------------------------
# the controller on hand-made partials
# ---------------------------------------------------------------------------
RPP, N_S, N_U = 512, 3, 1
CNT = float(RPP * (N_S + N_U))
T_END = 1.0


def scen(name, ratio=None, n1=0.0, nan_ok=False, **ctl):
    """One problem of a controller launch: the sum that makes sqrt(s / cnt) ``ratio`` and the block it starts from."""
    return dict(name=name, ratio=ratio, n1=n1, ctl=ctl, nan_ok=nan_ok)


MODE0 = [scen("d0 < 1e-5", 0.9e-5, 5.0), scen("d1 < 1e-5", 5.0, 0.9e-5), scen("regular", 8.0, 2.0),
         scen("resets", 3.0, 7.0, t=0.3, nsteps=9, done=1, nacc=3, ovf=1)]
MODE1 = [scen("both <= 1e-15", 0.0, h0=4e-3, d1=1e-16), scen("the 100 h0 cap", 2e-3, h0=1e-6, d1=3.0),
         scen("regular", 0.3, h0=0.01, d1=50.0)]
RATIOS = [scen("ratio 0", 0.0), scen("ratio 1e-8", 1e-8), scen("ratio 0.5", 0.5), scen("ratio 0.9", 0.9),
          scen("ratio 1 exactly", 1.0), scen("ratio 2", 2.0), scen("ratio 1e6", 1e6), scen("ratio inf", math.inf)]
RATIOS = [dict(s, ctl=dict(h=0.125, t=0.25, nacc=2, nsteps=4)) for s in RATIOS]
FINISH = [scen("ratio NaN", math.nan, nan_ok=True, h=0.125, t=0.25, nacc=2, nsteps=4),
          scen("t + h > t_end", 0.5, h=0.5, t=0.75, nacc=1, nsteps=3),
          scen("t + h == t_end", 0.5, h=0.25, t=0.75, nacc=1, nsteps=3),
          scen("ratio 1 at t_end", 1.0, h=0.25, t=0.75, nacc=0, nsteps=1),
          scen("rejected at t_end", 2.0, h=0.5, t=0.75, nacc=1, nsteps=3)]
CHAIN_SLOTS, CHAIN_LOG = 4, 6
CHAINED = [scen("accepted, goes on", 0.5, h=0.125, t=0.25, nacc=1, nsteps=2),
           scen("rejected", 2.0, h=0.125, t=0.25, nacc=1, nsteps=2),
           scen("finishes", 0.5, h=0.5, t=0.75, nacc=2, nsteps=5),
           scen("log full", 0.5, h=0.125, t=0.25, nacc=1, nsteps=CHAIN_LOG),
           scen("no slot left", 0.5, h=0.125, t=0.25, nacc=CHAIN_SLOTS - 1, nsteps=3),
           scen("already done", 0.5, h=0.125, t=0.25, nacc=1, nsteps=2, done=1),
           scen("ratio NaN", math.nan, nan_ok=True, h=0.125, t=0.25, nacc=2, nsteps=4),
           scen("ratio 1 at t_end", 1.0, h=0.25, t=0.75, nacc=0, nsteps=0)]


def sum_of(ratio, cnt):
    if ratio is None or math.isnan(ratio) or math.isinf(ratio):
        return ratio
    return Q.partial_for(ratio, cnt)


def spread(s, nblk, width, col):
    """A problem's (nblk, width) partials whose column ``col`` adds up to ``s`` exactly in any order: nblk = 3 ->
    s / 2, s / 4, s / 4; nblk = 70 -> s / 64 in blocks 3 .. 66 (two blocks per lane for the first lanes of the stride
    loop), zeros elsewhere."""
    out = torch.zeros(nblk, width, dtype=F64)
    if nblk == 3:
        out[:, col] = torch.tensor([s / 2, s / 4, s / 4], dtype=F64)
    else:
        out[3:67, col] = s / 64
    if isinstance(s, float) and (math.isnan(s) or math.isinf(s)):
        out[:, col] = 0.0
        out[1, col] = s
    back = out.float().double()
    assert bool(((back == out) | torch.isnan(out)).all()), "the partials are not float32 numbers"
    return out


def same(got, want, what, tol=1e-12):
    """Every double within ``tol`` relative of the reference's; NaN where it has NaN."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    for k, (a, b) in enumerate(zip(got, want)):
        if math.isnan(b):
            assert math.isnan(a), "%s [%d]: %r where NaN was left" % (what, k, a)
        else:
            assert a == b or abs(a - b) <= tol * abs(b), "%s [%d]: %.17g, the reference has %.17g" % (what, k, a, b)


def check_blocks(scens, before, got, want, what):
    """The 16 doubles of every problem: 1e-12 against the reference; what the reference left alone is bit-unchanged.  A
    NaN ratio: only that the attempt is not accepted and the solve neither ends nor advances."""
    for p, sc in enumerate(scens):
        lab = "%s: %s" % (what, sc["name"])
        if sc["nan_ok"]:
            assert got[p][Q.C_ACCEPT] == 0.0 and got[p][Q.C_DONE] == 0.0, lab
            assert got[p][Q.C_T] == before[p][Q.C_T] and got[p][Q.C_NACC] == before[p][Q.C_NACC], lab
            continue
        same(got[p], want[p], lab)
        for k in range(Q.CTL):
            if want[p][k] == before[p][k]:
                assert got[p][k] == before[p][k], "%s: field %d changed" % (lab, k)


def run_controller(entry, scens, mode, nblk=3, chained=False, pnorm=None):
    """One launch of ``entry`` ("dopri", "adj", "tiles") over ``scens``; returns what it left and what the reference
    leaves: (ctl, hslots, alog) each."""
    P = len(scens)
    rpp = 2240 if entry == "tiles" else RPP
    cnt = float(rpp * (N_S + N_U))
    width = 4 if entry == "adj" else 2
    part = torch.zeros(P, nblk, width, dtype=F64)
    for p, sc in enumerate(scens):
        part[p] += spread(sum_of(sc["ratio"], cnt), nblk, width, 0)
        part[p] += spread(sum_of(sc["n1"], cnt), nblk, width, 1)
        if entry == "adj":           # the adjoint part: a quarter of the y part's norms, so the y part leads
            part[p] += spread(sum_of(sc["ratio"], cnt) / 16, nblk, width, 2) if sc["ratio"] == sc["ratio"] else 0
    before = [Q.ctl_block(p, **sc["ctl"]) for p, sc in enumerate(scens)]
    ctl = out_buf(P, Q.CTL, torch.tensor(before, dtype=F64), dtype=F64)
    d_part = out_buf(P * nblk, width, part.float())
    n_slots, cap = (CHAIN_SLOTS, CHAIN_LOG) if chained else (0, 0)
    hs0 = torch.full((P, max(n_slots, 1)), NAN, dtype=F64)
    al0 = torch.full((P, max(cap, 1) * 3), NAN, dtype=F64)
    hslots, alog = out_buf(P, hs0.shape[1], hs0, dtype=F64), out_buf(P, al0.shape[1], al0, dtype=F64)
    pin = None
    if entry == "dopri":
        call("nlbac_dopri_control", d_part.data_ptr(), nblk, mode, N_S, N_U, rpp, P, T_END, ctl.data_ptr(), n_slots,
             hslots.data_ptr() if chained else None, alog.data_ptr() if chained else None, cap)
    elif entry == "adj":
        d_pn = None if pnorm is None else dev(torch.tensor(pnorm, dtype=F32))
        call("nlbac_adj_control", d_part.data_ptr(), nblk, mode, N_S, N_U, rpp, P, T_END, ptr(d_pn), ctl.data_ptr())
    else:
        pin = torch.full((P + 1, Q.CTL), SENT, dtype=F64).pin_memory()
        ch = lib().RkChain()
        ch.partials, ch.ctl_w, ch.norm_mode, ch.norm_defer, ch.t_end = d_part.data_ptr(), ctl.data_ptr(), 2, 1, T_END
        ch.n_slots, ch.alog_cap, ch.ctl_host, ch.ctl_seq = n_slots, cap, pin.data_ptr(), 5.0
        if chained:
            ch.hslots, ch.alog = hslots.data_ptr(), alog.data_ptr()
        call("nlbac_dopri_control_tiles", C.byref(ch), N_S, N_U, rpp, P)
    torch.cuda.synchronize()
    assert torch.equal(read(d_part, P * nblk, width, "partials"), part.float().reshape(P * nblk, width)) or bool(
        torch.isnan(part).any())
    got = (read(ctl, P, Q.CTL, "ctl").numpy(), read(hslots, P, hs0.shape[1], "hslots").numpy(),
           read(alog, P, al0.shape[1], "alog").numpy().reshape(P, -1, 3))
    want_c, want_h, want_a = [], [], []
    f32part = part.float().double()
    for p, sc in enumerate(scens):
        sums = [float(f32part[p, :, k].sum()) for k in range(width)]
        if entry == "adj":
            n0, n1 = Q.adj_norms(sums, rpp, N_S + N_U, None if pnorm is None else [T.f32(v) for v in pnorm])
        else:
            n0, n1 = float(np.sqrt(np.float64(sums[0]) / cnt)), float(np.sqrt(np.float64(sums[1]) / cnt))
        skip = {"dopri": chained, "adj": True, "tiles": True}[entry]
        c, h, a = Q.control_launch(mode, n0, n1, before[p], T_END, n_slots, list(hs0[p].numpy()) if chained else None,
                                   [list(r) for r in al0[p].reshape(-1, 3).numpy()] if chained else None, cap, skip)
        want_c.append(c)
        want_h.append(h if chained else list(hs0[p].numpy()))
        want_a.append(a if chained else [list(r) for r in al0[p].reshape(-1, 3).numpy()])
    if pin is not None:
        for p, sc in enumerate(scens):
            if before[p][Q.C_DONE] > 0:
                assert bool((pin[p] == SENT).all()), "the host copy of a finished problem was written"
            else:
                assert pin[p, Q.C_SEQ] == 5.0 and np.array_equal(pin[p, :Q.C_SEQ].numpy(), got[0][p, :Q.C_SEQ], equal_nan=True)
        assert bool((pin[P] == SENT).all())
    return before, got, (want_c, want_h, want_a)


def check_launch(entry, scens, mode, what, **kw):
    before, got, want = run_controller(entry, scens, mode, **kw)
    check_blocks(scens, before, got[0], want[0], "%s %s" % (entry, what))
    for p, sc in enumerate(scens):
        if sc["nan_ok"]:
            continue
        same(got[1][p], want[1][p], "%s %s: %s: hslots" % (entry, what, sc["name"]))
        same(got[2][p], want[2][p], "%s %s: %s: attempt log" % (entry, what, sc["name"]))
    return before, got, want


def test_dopri_control_initial_step_branches():
    before, got, want = check_launch("dopri", MODE0, 0, "mode 0")
    assert [got[0][p][Q.C_H0] == 1e-6 for p in range(4)] == [True, True, False, False]
    for p in range(4):
        assert all(got[0][p][k] == 0.0 for k in (Q.C_T, Q.C_NSTEPS, Q.C_DONE, Q.C_NACC, Q.C_OVF))
    before, got, want = check_launch("dopri", MODE1, 1, "mode 1")
    assert got[0][0][Q.C_H] == 4e-3 * 1e-3 and got[0][1][Q.C_H] == 100.0 * 1e-6 and got[0][2][Q.C_H] < 1.0


def test_dopri_control_attempt_branches():
    before, got, want = check_launch("dopri", RATIOS, 2, "mode 2")
    c = got[0]
    assert [c[p][Q.C_ACCEPT] for p in range(8)] == [1, 1, 1, 1, 1, 0, 0, 0]
    assert c[0][Q.C_H] == 1.25 and c[1][Q.C_H] == 1.25 and c[3][Q.C_H] == 0.125           # fac 10, the clamp at 10, the floor at 1
    assert c[4][Q.C_RATIO] == 1.0 and c[4][Q.C_H] == 0.125 * 0.9                            # ratio 1.0 exactly: accepted
    assert c[6][Q.C_H] == 0.125 * 0.2 and c[7][Q.C_H] == 0.125 * 0.2                         # the clamp at 0.2; inf
    before, got, want = check_launch("dopri", FINISH, 2, "finishing")
    c = got[0]
    for p in (1, 2, 3):
        assert c[p][Q.C_DONE] == 1.0 and all(c[p][k] == before[p][k] for k in (Q.C_T, Q.C_H, Q.C_NACC))
    assert c[1][Q.C_X] == 0.5 and c[2][Q.C_X] == 1.0 and c[3][Q.C_X] == 1.0
    assert c[4][Q.C_DONE] == 0.0 and c[4][Q.C_ACCEPT] == 0.0


@pytest.mark.parametrize("entry", ["dopri", "tiles"])
def test_control_chained(entry):
    """One launch of eight problems: accepted, rejected, finishing, log full, no slot left, already done, NaN, and
    ratio 1 landing on t_end; step slots, attempt log (and, for the tile form, the host's copy)."""
    before, got, want = check_launch(entry, CHAINED, 2, "chained", chained=True, nblk=70 if entry == "tiles" else 3)
    c, hs, al = got
    assert c[0][Q.C_T] == 0.375 and c[0][Q.C_NACC] == 2 and hs[0][1] == 0.125 and list(al[0][2]) == [0.125, c[0][Q.C_RATIO], 1.0]
    assert bool(np.isnan(hs[1]).all()) and list(al[1][2]) == [0.125, c[1][Q.C_RATIO], 0.0]
    assert c[2][Q.C_DONE] == 1.0 and hs[2][2] == 0.5
    assert bool(np.isnan(al[3]).all()) and c[3][Q.C_NSTEPS] == CHAIN_LOG + 1              # nothing past the log
    assert c[4][Q.C_OVF] == 1.0 and c[4][Q.C_DONE] == 1.0 and c[4][Q.C_NACC] == CHAIN_SLOTS - 1 and c[4][Q.C_T] == 0.375
    assert list(c[5]) == before[5] and bool(np.isnan(hs[5]).all()) and bool(np.isnan(al[5]).all())
    assert c[7][Q.C_DONE] == 1.0 and c[7][Q.C_X] == 1.0 and hs[7][0] == 0.25


def test_control_tiles_unchained_ratios():
    check_launch("tiles", RATIOS, 2, "mode 2", nblk=70)
    check_launch("tiles", FINISH, 2, "finishing", nblk=70)


@pytest.mark.parametrize("pnorm", [None, (0.01, 0.02), (40.0, 50.0)], ids=["none", "below", "dominating"])
def test_adj_control(pnorm):
    """``pnorm`` NULL, below the row norms and dominating them (both entries in mode 0)."""
    before, got, want = check_launch("adj", MODE0[2:], 0, "mode 0 pnorm %s" % (pnorm,), pnorm=pnorm)
    if pnorm and pnorm[0] > 8.0:
        assert got[0][0][Q.C_D0] == 40.0 and got[0][0][Q.C_D1] == 50.0
    else:
        assert got[0][0][Q.C_D0] == 8.0 and got[0][0][Q.C_D1] == 2.0
    check_launch("adj", MODE1, 1, "mode 1 pnorm %s" % (pnorm,), pnorm=pnorm)
    scens = [s for s in RATIOS if not math.isinf(s["ratio"])] + FINISH + [CHAINED[5]]
    for k in range(0, len(scens), 8):
        before, got, want = check_launch("adj", scens[k:k + 8], 2, "mode 2 pnorm %s" % (pnorm,), pnorm=pnorm)
        if pnorm and pnorm[0] > 8.0:
            assert all(got[0][p][Q.C_RATIO] == 40.0 for p, s in enumerate(scens[k:k + 8])
                       if not s["nan_ok"] and not s["ctl"].get("done") and s["ratio"] < 40.0)


# ---------------------------------------------------------------------------
# fused norm + control
# ---------------------------------------------------------------------------
def device_norms(part, s, adjoint):
    """(n0, n1) per problem from the partials a launch left, summed in double."""
    out = []
    for p in range(s.P):
        if adjoint:
            out.append(Q.adj_norms([float(v) for v in part[p].double().sum(0)], s.rows, s.n_s + s.n_u))
        else:
            out.append((Q.rms_of(part[p, :, 0].numpy(), s.rows, s.n_s + s.n_u),
                        Q.rms_of(part[p, :, 1].numpy(), s.rows, s.n_s + s.n_u)))
    return out


def fused_launch(c, s, adjoint, before, chain=None, pin=None, seq=0.0, slot_args=None):
    """One fused launch of case ``c`` from the blocks ``before``; returns (partials, ctl, tickets)."""
    nb, width = nblk_of(s.rows), 4 if adjoint else 2
    d = {k: dev(v) for k, v in c.inputs.items()}
    if "u" in d and s.n_u == 0:
        d["u"] = dev(torch.zeros(1))
    part = out_buf(s.P * nb, width)
    tickets = dev(torch.zeros(9, dtype=torch.int32))
    ctl = out_buf(s.P, Q.CTL, torch.tensor(before, dtype=F64), dtype=F64)
    outs = []
    for _ in range(2):       # the second launch starts from the same blocks with the tickets the first one left
        ctl[:s.P] = dev(torch.tensor(before, dtype=F64))
        if adjoint:
            call("nlbac_adj_norm_control", ptr(d.get("a")), ptr(d.get("b")), ptr(d.get("Z0")), ptr(d.get("Z1")),
                 ptr(d.get("u")), c.meta.mode, s.rtol, s.atol, s.n_s, s.n_u, s.rows, s.P, Q.FUSED_T_END, None, part.data_ptr(),
                 tickets.data_ptr(), ctl.data_ptr(), ptr(pin), seq)
        else:
            a, b, y0, y1, u = (ptr(d.get(k)) for k in ("a", "b", "y0", "y1", "u"))
            if slot_args:
                a, y0, y1 = slot_args
            if chain is not None:
                chain.ctl = ctl.data_ptr()
            call("nlbac_dopri_norm_control", a, b, y0, y1, u, c.meta.mode, s.rtol, s.atol, s.n_s, s.n_u, s.rows, s.P,
                 Q.FUSED_T_END, part.data_ptr(), tickets.data_ptr(), ctl.data_ptr(), None if chain is None else C.byref(chain))
        torch.cuda.synchronize()
        assert bool((tickets.cpu() == 0).all()), "the tickets were not left at zero"
        outs.append((read(part, s.P * nb, width, "partials").reshape(s.P, nb, width).clone(),
                     read(ctl, s.P, Q.CTL, "ctl").numpy().copy()))
    assert np.array_equal(outs[0][1], outs[1][1], equal_nan=True), "a second identical launch left other blocks"
    assert torch.equal(outs[0][0], outs[1][0])
    return outs[0]


@pytest.mark.parametrize("adjoint", [False, True], ids=["dopri", "adjoint"])
@pytest.mark.parametrize("rows", Q.ROWS)
def test_fused_norm_control(rows, adjoint):
    """(a) the partials the launch left are within the bar of the float64 sums; (b) the control block is the
    controller's on those very partials, to 1e-12."""
    for c in by_rows(Q.adj_norm_cases() if adjoint else Q.norm_cases(), rows):
        s = (Q.adj_case if adjoint else Q.state_case)(*c.meta.key)
        mode = c.meta.mode
        before = [b[0] for b in Q.fused_reference(c.meta.key, mode, adjoint)]
        part, ctl = fused_launch(c, s, adjoint, before)
        compare(c, dict(partials=part), " fused%s" % (" adjoint" if adjoint else ""))
        norms = device_norms(part, s, adjoint)
        want = [Q.control_launch(mode, norms[p][0], norms[p][1], before[p], Q.FUSED_T_END, skip_done=adjoint)[0]
                for p in range(s.P)]
        for p in range(s.P):
            same(ctl[p], want[p], "%s mode %d problem %d" % (c.label, mode, p))


def test_fused_norm_control_chain():
    """rpp = 600, P = 3 with a chain: step slots, attempt log and the host's copy in pinned memory."""
    key = (600, 3, 6, 2, 0)
    s = Q.state_case(*key)
    c = [c for c in Q.norm_cases() if c.meta.key == key and c.meta.mode == 2][0]
    before = [b[0] for b in Q.fused_reference(key, 2, False)]
    slots = [int(b[Q.C_NACC]) for b in before]
    assert slots == [0, 1, 2]
    E, Y1, y0 = slot_buffers(s, slots, CHAIN_SLOTS)
    hs0 = torch.full((s.P, CHAIN_SLOTS), NAN, dtype=F64)
    al0 = torch.full((s.P, CHAIN_LOG * 3), NAN, dtype=F64)
    hslots, alog = out_buf(s.P, CHAIN_SLOTS, hs0, dtype=F64), out_buf(s.P, CHAIN_LOG * 3, al0, dtype=F64)
    pin = torch.full((s.P + 1, Q.CTL), SENT, dtype=F64).pin_memory()
    ch = lib().RkChain()
    ch.slot_floats, ch.norm_mode, ch.n_slots, ch.t_end = s.n * s.n_s, 2, CHAIN_SLOTS, Q.FUSED_T_END
    ch.hslots, ch.alog, ch.alog_cap, ch.ctl_host, ch.ctl_seq = hslots.data_ptr(), alog.data_ptr(), CHAIN_LOG, pin.data_ptr(), 5.0
    part, ctl = fused_launch(c, s, False, before, chain=ch, slot_args=(E.data_ptr(), y0.data_ptr(), Y1.data_ptr()))
    compare(c, dict(partials=part), " chain")
    norms = device_norms(part, s, False)
    hs, al = read(hslots, s.P, CHAIN_SLOTS, "hslots").numpy(), read(alog, s.P, CHAIN_LOG * 3, "alog").numpy()
    outcomes = []
    for p in range(s.P):
        w, h, a = Q.control_launch(2, norms[p][0], norms[p][1], before[p], Q.FUSED_T_END, CHAIN_SLOTS, list(hs0[p].numpy()),
                                   [list(r) for r in al0[p].reshape(-1, 3).numpy()], CHAIN_LOG, True)
        same(ctl[p], w, "chain problem %d" % p)
        same(hs[p], h, "chain problem %d hslots" % p)
        same(al[p], a, "chain problem %d attempt log" % p)
        outcomes.append((w[Q.C_ACCEPT], w[Q.C_DONE]))
        assert pin[p, Q.C_SEQ] == 5.0 and np.array_equal(pin[p, :Q.C_SEQ].numpy(), ctl[p][:Q.C_SEQ])
        assert ctl[p][Q.C_SEQ] == before[p][Q.C_SEQ]
    assert outcomes == [(1.0, 1.0), (0.0, 0.0), (1.0, 0.0)] and bool((pin[s.P] == SENT).all())


def test_fused_adjoint_host_copy():
    key = (600, 3, 6, 2, 0)
    s = Q.adj_case(*key)
    c = [c for c in Q.adj_norm_cases() if c.meta.key == key and c.meta.mode == 2][0]
    before = [b[0] for b in Q.fused_reference(key, 2, True)]
    pin = torch.full((s.P + 1, Q.CTL), SENT, dtype=F64).pin_memory()
    part, ctl = fused_launch(c, s, True, before, pin=pin, seq=5.0)
    for p in range(s.P):
        assert pin[p, Q.C_SEQ] == 5.0 and np.array_equal(pin[p, :Q.C_SEQ].numpy(), ctl[p][:Q.C_SEQ])
    assert bool((pin[s.P] == SENT).all())


# ---------------------------------------------------------------------------
# the interpolant
# ---------------------------------------------------------------------------
def hx_block(h, x):
    """Control blocks whose C_HUSED / C_X hold the doubles (not float32 numbers, mostly): the launch casts them."""
    c = torch.full((len(h), Q.CTL), NAN, dtype=F64)
    c[:, Q.C_HUSED], c[:, Q.C_X] = torch.tensor(h, dtype=F64), torch.tensor(x, dtype=F64)
    return dev(c)


def out_map(l, p=None, dp=None, dp2=None, x=None):
    m = lib().OutMap()
    m.kind, m.l, m.p, m.dp, m.dp2, m.x = 1, l, ptr(p), ptr(dp), ptr(dp2), ptr(x)
    return m


def interp_fwd(c, from_ctl):
    s, m, t = Q.state_case(*c.meta.key), c.meta, c.inputs
    y0, y1, Kd = dev(t["y0"]), dev(t["y1"]), dev(t["K"])
    out = out_buf(s.n, s.n_s)
    p = out_buf(s.n, 2) if m.l is not None else None
    om = out_map(m.l, p=p) if m.l is not None else None
    blk = hx_block(m.h, m.x) if from_ctl else None
    call("nlbac_dopri_interp_fwd", y0.data_ptr(), y1.data_ptr(), Kd.data_ptr(), None if from_ctl else fptr(m.h),
         None if from_ctl else fptr(m.x), ptr(blk), s.P, s.rows, s.n_s, out.data_ptr(), 0, None if om is None else C.byref(om))
    torch.cuda.synchronize()
    got = dict(out=read(out, s.n, s.n_s, "out"))
    if p is not None:
        got["p"] = read(p, s.n, 2, "p")
    return got


def interp_bwd(c, from_ctl):
    s, m, t = Q.state_case(*c.meta.key), c.meta, c.inputs
    dK, dy0, dy1 = out_buf(7 * s.n, s.n_s), out_buf(s.n, s.n_s), out_buf(s.n, s.n_s)
    d = {k: dev(v) for k, v in t.items() if "@" not in k}
    om = out_map(m.l, dp=d["dps"], dp2=d.get("dps2"), x=d["xo"]) if m.l is not None else None
    blk = hx_block(m.h, m.x) if from_ctl else None
    call("nlbac_dopri_interp_bwd", ptr(d.get("dout")), None if from_ctl else fptr(m.h), None if from_ctl else fptr(m.x),
         ptr(blk), s.P, s.rows, s.n_s, dy0.data_ptr(), dy1.data_ptr(), dK.data_ptr(), 0, None if om is None else C.byref(om))
    torch.cuda.synchronize()
    return dict(dy0=read(dy0, s.n, s.n_s, "dy0"), dy1=read(dy1, s.n, s.n_s, "dy1"),
                dK=read(dK, 7 * s.n, s.n_s, "dK").reshape(7, s.n, s.n_s))


@pytest.mark.parametrize("rows", Q.ROWS)
def test_dopri_interp(rows):
    for c in by_rows(Q.interp_cases(), rows):
        s = Q.state_case(*c.meta.key)
        run = interp_bwd if c.op.endswith("bwd") else interp_fwd
        got = run(c, False)
        ref, bar = compare(c, got, " by value")
        again = run(c, True)
        compare_ref(c.op, ref, bar, again, c.label + " from ctl")
        for k in got:
            assert torch.equal(got[k], again[k]), "%s %s: by value and from the control block differ" % (c.op, k)
        if c.op in ("interp", "interp_map"):
            for p, x in enumerate(c.meta.x):
                if x == 0.0:
                    r = slice(p * s.rows, (p + 1) * s.rows)
                    assert torch.equal(got["out"][r], c.inputs["y0"][r]), "x = 0 is not y0"


def test_dopri_interp_step_slots():
    """The slot form: problem 0 in slot 0 on the caller's y0, problem 1 in slot 2 on slot 1's y1; the backward writes
    into the same slots."""
    key = (257, 3, 6, 2, 0)
    s = Q.state_case(*key)
    P, n, nn = 2, 2 * s.rows, 2 * s.rows * s.n_s
    t = dict(y0=s.y0[:n], y1=s.y1[:n], K=s.K[:, :n].contiguous())
    h, x = [0.05, 0.7], [0.37, 1e-6]
    slots, n_slots, sf = (0, 2), 3, 8 * nn
    buf = torch.full((n_slots, 8, n, s.n_s), NAN)        # per slot: K (7 stages), then y1
    y0 = torch.full((n, s.n_s), NAN)
    for p, k in enumerate(slots):
        r = slice(p * s.rows, (p + 1) * s.rows)
        buf[k, :7, r], buf[k, 7, r] = t["K"][:, r], t["y1"][r]
        if k == 0:
            y0[r] = t["y0"][r]
        else:
            buf[k - 1, 7, r] = t["y0"][r]
    d_buf, d_y0 = dev(buf), dev(y0)
    ctl = torch.tensor([Q.ctl_block(p, nacc=k, hused=h[p], x=x[p]) for p, k in enumerate(slots)], dtype=F64)
    d_ctl = dev(ctl)
    out = out_buf(n, s.n_s)
    call("nlbac_dopri_interp_fwd", d_y0.data_ptr(), d_buf.data_ptr() + 4 * 7 * nn, d_buf.data_ptr(), None, None,
         d_ctl.data_ptr(), P, s.rows, s.n_s, out.data_ptr(), sf, None)
    torch.cuda.synchronize()
    fn = lambda q: Q.interp(q, h, x, s.rows)
    inputs = Q.per_use(t, ("y0", "y1", "K"))
    ref, bar = Q.reference_and_bar("interp", fn, inputs)
    compare_ref("interp", ref, bar, dict(out=read(out, n, s.n_s, "out")), "step slots")

    g = T.randn(T.gen(77), n, s.n_s)
    d_g = dev(g)
    grads = torch.full((n_slots + 1, 9, n, s.n_s), NAN)  # per slot: dK (7 stages), dy0, dy1; a guard slot
    grads[n_slots] = SENT
    d_gr = dev(grads)
    call("nlbac_dopri_interp_bwd", d_g.data_ptr(), None, None, d_ctl.data_ptr(), P, s.rows, s.n_s,
         d_gr.data_ptr() + 4 * 7 * nn, d_gr.data_ptr() + 4 * 8 * nn, d_gr.data_ptr(), 9 * nn, None)
    torch.cuda.synchronize()
    gr = d_gr.cpu()
    assert bool((gr[n_slots] == SENT).all())
    got = dict(dK=torch.empty(7, n, s.n_s), dy0=torch.empty(n, s.n_s), dy1=torch.empty(n, s.n_s))
    written = torch.zeros(n_slots, 9, n, s.n_s, dtype=torch.bool)
    for p, k in enumerate(slots):
        r = slice(p * s.rows, (p + 1) * s.rows)
        got["dK"][:, r], got["dy0"][r], got["dy1"][r] = gr[k, :7, r], gr[k, 7, r], gr[k, 8, r]
        written[k, :, r] = True
    assert bool(torch.isnan(gr[:n_slots][~written]).all()), "the backward wrote outside its slots"
    refb, barb = Q.reference_and_bar("interp_bwd", lambda q: Q.interp_bwd(q, h, x, s.rows),
                                     Q.per_use(dict(dout=g), ("dout",), Q.GRAD_USES))
    compare_ref("interp_bwd", refb, barb, got, "step slots")
    assert torch.equal(d_ctl.cpu(), ctl)


@pytest.mark.parametrize("key", [(257, 3, 6, 2, 0), (600, 3, 3, 2, 0)], ids=Q.key_label)
def test_dopri_interp_kernels_are_adjoint(key):
    """<g, fwd(v)> and <bwd(g), v>, both in float64 from the device's results, agree to the sum of the two bars."""
    fc = [c for c in Q.interp_cases() if c.meta.key == key and c.op == "interp"][0]
    bc = [c for c in Q.interp_cases() if c.meta.key == key and c.op == "interp_bwd"][0]
    out = interp_fwd(fc, False)["out"].double()
    gr = interp_bwd(bc, False)
    g = bc.inputs["dout"].double()
    v = {k: fc.inputs[k].double() for k in ("y0", "y1", "K")}
    lhs = float((g * out).sum())
    rhs = float((gr["dy0"].double() * v["y0"]).sum() + (gr["dy1"].double() * v["y1"]).sum() + (gr["dK"].double() * v["K"]).sum())
    _, bar_f = Q.reference_and_bar(fc.op, fc.fn, fc.inputs)
    _, bar_b = Q.reference_and_bar(bc.op, bc.fn, bc.inputs)
    bound = float((g.abs() * bar_f["out"]).sum() + (bar_b["dy0"] * v["y0"].abs()).sum() + (bar_b["dy1"] * v["y1"].abs()).sum()
                  + (bar_b["dK"] * v["K"].abs()).sum())
    print("device / bar  interp adjoint   <g, fwd v> - <bwd g, v> = %.3e, the two bars allow %.3e: %.3f" % (
        lhs - rhs, bound, abs(lhs - rhs) / bound))
    assert abs(lhs - rhs) <= bound


# ---------------------------------------------------------------------------
# adjoint glue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", Q.ROWS)
def test_adj_pack_unpack(rows):
    for (n_s, n_u) in Q.DIMS:
        g = T.gen(60 + rows + n_s)
        n, W = 2 * rows, 2 * n_s + n_u
        y, ax = T.randn(g, n, n_s), T.randn(g, n, n_s)
        Z, d_y, d_ax = out_buf(n, W), dev(y), dev(ax)
        call("nlbac_adj_pack", d_y.data_ptr(), d_ax.data_ptr(), n_s, n_u, n, Z.data_ptr())
        Zr = T.randn(g, n, W)
        d_Zr = dev(Zr)
        outs = []
        for want_dy0, want_du in ((True, True), (True, False), (False, True)):
            dy0 = out_buf(n, n_s) if want_dy0 else None
            du = out_buf(n, max(n_u, 1)) if want_du else None
            call("nlbac_adj_unpack", d_Zr.data_ptr(), n_s, n_u, n, ptr(dy0), ptr(du))
            outs.append((dy0, du))
        torch.cuda.synchronize()
        assert torch.equal(read(Z, n, W, "Z"), Q.pack(y, ax, n_u))
        a_x, a_u = Q.unpack(Zr, n_s, n_u)
        for dy0, du in outs:
            if dy0 is not None:
                assert torch.equal(read(dy0, n, n_s, "dy0"), a_x)
            if du is not None:
                assert torch.equal(read(du, n, n_u, "du"), a_u)


@pytest.mark.parametrize("rpp,w", [(1, 8), (255, 8), (257, 14), (600, 20)])
@pytest.mark.parametrize("with_dst1", [False, True])
def test_adj_commit(rpp, w, with_dst1):
    """Three problems: accepted and running, rejected, accepted and done.  Only the first one's rows change."""
    g = T.gen(70 + rpp)
    n = 3 * rpp
    ctl = torch.tensor([Q.ctl_block(0, accept=1, done=0), Q.ctl_block(1, accept=0, done=0),
                        Q.ctl_block(2, accept=1, done=1)], dtype=F64)
    d0, s0, d1, s1 = (T.randn(g, n, w) for _ in range(4))
    dst0, dst1, d_ctl, src0, src1 = out_buf(n, w, d0), out_buf(n, w, d1), dev(ctl), dev(s0), dev(s1)
    call("nlbac_adj_commit", d_ctl.data_ptr(), rpp, n, w, dst0.data_ptr(), src0.data_ptr(),
         dst1.data_ptr() if with_dst1 else None, src1.data_ptr() if with_dst1 else None)
    torch.cuda.synchronize()
    assert torch.equal(read(dst0, n, w, "dst0"), Q.commit(ctl.tolist(), rpp, d0, s0))
    assert torch.equal(read(dst1, n, w, "dst1"), Q.commit(ctl.tolist(), rpp, d1, s1) if with_dst1 else d1)
    assert not torch.equal(Q.commit(ctl.tolist(), rpp, d0, s0), d0)


@pytest.mark.parametrize("accept,done", [(1, 0), (0, 0), (1, 1)])
def test_adj_commit_parameter_form(accept, done):
    """w = 4, rows_per_problem = n_rows: one problem, the whole vector moves or none of it."""
    g = T.gen(75)
    n = 379
    ctl = torch.tensor([Q.ctl_block(0, accept=accept, done=done)], dtype=F64)
    d0, s0, d1, s1 = (T.randn(g, n, 4) for _ in range(4))
    dst0, dst1, d_ctl, src0, src1 = out_buf(n, 4, d0), out_buf(n, 4, d1), dev(ctl), dev(s0), dev(s1)
    call("nlbac_adj_commit", d_ctl.data_ptr(), n, n, 4, dst0.data_ptr(), src0.data_ptr(), dst1.data_ptr(), src1.data_ptr())
    torch.cuda.synchronize()
    moved = accept and not done
    assert torch.equal(read(dst0, n, 4, "dst0"), s0 if moved else d0)
    assert torch.equal(read(dst1, n, 4, "dst1"), s1 if moved else d1)


@pytest.mark.parametrize("h_dev", [False, True], ids=["h_host", "h_dev"])
def test_adj_param_norm(h_dev):
    segs, N = Q.segments()
    seg_off = dev(torch.tensor([o for o, _ in segs], dtype=torch.int32))
    seg_len = dev(torch.tensor([ln for _, ln in segs], dtype=torch.int32))
    for c in Q.param_cases():
        m, t = c.meta, c.inputs
        th0, Kd = dev(t["th0"]), dev(t["K"])
        th1, pseg, pnorm = out_buf(N, 1), out_buf(2 * len(segs), 1), out_buf(2, 1)
        ticket = dev(torch.zeros(2, dtype=torch.int32))
        hd = dev(torch.tensor([m.h, NAN], dtype=F64)) if h_dev else None
        args = lambda ctl: (m.mode, th0.data_ptr(), Kd.data_ptr(), N, 7, fptr(Q.C_SOL), fptr(Q.C_ERR),
                            None if h_dev else fptr([m.h]), ptr(hd), seg_off.data_ptr(), seg_len.data_ptr(), len(segs),
                            Q.TOLS[0][0], Q.TOLS[0][1], ptr(ctl), th1.data_ptr(), pseg.data_ptr(), ticket.data_ptr(),
                            pnorm.data_ptr())
        if m.mode == 2:      # a finished solve: nothing is written
            done = dev(torch.tensor([Q.ctl_block(0, done=1)], dtype=F64))
            call("nlbac_adj_param_norm", *args(done))
            torch.cuda.synchronize()
            assert bool(torch.isnan(read(th1, N, 1, "th1")).all()) and bool(torch.isnan(read(pnorm, 2, 1, "pnorm")).all())
            assert bool((ticket.cpu() == 0).all())
        running = dev(torch.tensor([Q.ctl_block(0, done=0)], dtype=F64)) if m.mode == 2 else None
        call("nlbac_adj_param_norm", *args(running))
        torch.cuda.synchronize()
        assert bool((ticket.cpu() == 0).all()), "the ticket was not left at zero"
        got = dict(pnorm=read(pnorm, 2, 1, "pnorm")[:, 0])
        full = read(th1, N, 1, "th1")[:, 0]
        inside = torch.zeros(N, dtype=torch.bool)
        for off, ln in segs:
            inside[off:off + ln] = True
        if m.mode == 2:
            got["th1"] = full[inside]
            assert bool(torch.isnan(full[~inside]).all()), "th1 was written in a gap"
        else:
            assert bool(torch.isnan(full).all())
        compare(c, got, " mode%d %s" % (m.mode, "h_dev" if h_dev else "h_host"))


def test_adj_param_norm_keeps_a_nan():
    """A tensor whose stage derivative is not a number: the maximum over the tensors is NaN in that column, not the
    largest of the others (the mixed norm then is NaN and the controller does not accept the step)."""
    segs, N = Q.segments()
    c = [c for c in Q.param_cases() if c.meta.mode == 0 and c.meta.big == 3][0]
    Ks = c.inputs["K"].clone()
    Ks[0, segs[1][0] + 7] = NAN
    th0, Kd = dev(c.inputs["th0"]), dev(Ks)
    seg_off = dev(torch.tensor([o for o, _ in segs], dtype=torch.int32))
    seg_len = dev(torch.tensor([ln for _, ln in segs], dtype=torch.int32))
    pseg, pnorm, ticket = out_buf(2 * len(segs), 1), out_buf(2, 1), dev(torch.zeros(2, dtype=torch.int32))
    call("nlbac_adj_param_norm", 0, th0.data_ptr(), Kd.data_ptr(), N, 7, None, None, None, None, seg_off.data_ptr(),
         seg_len.data_ptr(), len(segs), Q.TOLS[0][0], Q.TOLS[0][1], None, None, pseg.data_ptr(), ticket.data_ptr(),
         pnorm.data_ptr())
    torch.cuda.synchronize()
    got = read(pnorm, 2, 1, "pnorm")[:, 0]
    want = Q.param_norm(0, dict(th0=c.inputs["th0"].double(), K=Ks.double()), segs, 0.0, *Q.TOLS[0])["pnorm"]
    assert math.isnan(float(want[1])) and math.isnan(float(got[1]))
    assert abs(float(got[0]) - float(want[0])) <= 1e-4 * float(want[0])
