"""Float64 references, shared cases and the comparator for the dopri5 step control and the per-row RK glue:
``csrc/ode_kernels.hip`` (top of the file through ``nlbac_dopri_interp_bwd``), ``csrc/ode_control.h`` and the per-row
glue of ``csrc/node_adjoint_kernels.hip``.  Imports without a GPU.

References.  One plain function per operation, in the formulas' own form, run in the dtype of the tensors it is
handed: float64 is the reference, float32 the same formulas at the kernels' precision (what fixes ``K`` below).  Tensor
inputs are the float32 tensors the device gets, cast up.  Scalars the ABI takes as ``float`` are rounded to float32
(``f32``); a product the kernels form between two float scalars before it meets a tensor (``coef_j * h``, ``cm_j * h``) is
formed in float32 too (``fprod``), which is also how the oracle forms it.  Backward references are
``torch.autograd.grad`` of the forward ones.  The controller (``control``) is the state machine of
``dopri_control_vals`` in Python floats, which are doubles.

Block sums.  The float32 reference of a block sum adds its rows one after the other (``_block_sums``): the least
accurate order a kernel could use, so the bar covers whatever tree the kernel sums in.

Comparator (``task_kernels_common.reference_and_bar`` with ``k=``).  An element may differ from the float64 reference
by at most

    bar = K * ( max over 8 seeded draws of |f64(x (1 + d)) - f64(x)| + 2^-24 |f64(x)| ),   d ~ U[-2^-23, 2^-23]

``K`` comes from the reference alone: the smallest power of two for which the float32 evaluation of the same reference
stays within HALF the bar on every case below (``test_ode_control_host.py`` asserts it).  It is never adjusted from a
device result.  Every tensor also meets ``common.vec_close(..., 1e-4)``.

The interpolant.  Its polynomial form reads y0, y1 and y_mid once per coefficient a, b, c, and the reads cancel: at
x = 1 the value is y1 and its derivative with respect to y0 and K is identically zero, while a float32 evaluation is
left with the rounding of terms of size 32 |y|.  A bar that follows the value's sensitivity alone is zero there and no
``K`` exists.  So the comparator is handed one copy of each tensor per read (``per_use``): it perturbs every read on
its own and the bar follows the formula's sensitivity to a rounding of its terms; the copies are equal, so the
reference is what it was.  The backward's dy0, dy1, dK are one gradient and meet ``vec_close`` as one vector.  The
shared step is a real one: y1 = y0 + h sum_j c_sol_j K_j with the case's own h, K_0 = f0, K_6 = f1.

NaN.  The published algorithm leaves a NaN error norm unspecified; the one property held is that it is never accepted.
The adjoint's mixed norm therefore keeps a NaN of any of its parts (``_max_keep_nan``).

``K`` and the worst float32-reference / bar ratio (CPU), then the worst device / bar ratio (MI355X), per operation:

    operation                K   float32 reference   device
    affine_fwd                4   0.275               0.219
    affine_bwd                4   0.353               0.308
    rk_combine                4   0.488               0.455
    rk_stage_bwd              4   0.442               0.378
    norm_sums0               32   0.358               0.051
    norm_sums1                2   0.382               0.349
    norm_sums2               32   0.289               0.039
    adj_norm_sums0           32   0.375               0.063
    adj_norm_sums1            4   0.439               0.167
    adj_norm_sums2           32   0.274               0.044
    interp                    8   0.421               0.421
    interp_bwd               16   0.279               0.220
    interp_map                8   0.454               0.454
    interp_map_bwd           16   0.362               0.181
    param_norm0               8   0.380               0.077
    param_norm1               8   0.286               0.011
    param_norm2               4   0.344               0.344
"""
import functools
import math
import types

import numpy as np
import torch

import task_kernels_common as T
from task_kernels_common import F64, f32, gen, randn

# operation -> K (the table above)
K = {"affine_fwd": 4, "affine_bwd": 4, "rk_combine": 4, "rk_stage_bwd": 4,
     "norm_sums0": 32, "norm_sums1": 2, "norm_sums2": 32,
     "adj_norm_sums0": 32, "adj_norm_sums1": 4, "adj_norm_sums2": 32,
     "interp": 8, "interp_bwd": 16, "interp_map": 8, "interp_map_bwd": 16,
     "param_norm0": 8, "param_norm1": 8, "param_norm2": 4}

# the control block (csrc/ode_control.h)
CTL = 16
C_H, C_T, C_RATIO, C_ACCEPT, C_DONE, C_X, C_H0, C_D0, C_D1, C_D2, C_NSTEPS, C_HUSED, C_NACC, C_OVF = range(14)
C_SEQ = 15
NO_SLOTS = 1 << 30

ROWS = T.ROWS                                   # rows per problem: ragged last block, 1 / 2 / 3 blocks
DIMS = ((3, 2), (6, 2), (8, 4), (10, 0))        # (n_s, n_u); 10 is the single-net width (no per-row arrays: rk_combine, norms)
MAGS = (1e-3, 1.0, 1e3)
TOLS = ((1e-5, 1e-7), (1e-3, 1e-6))             # (rtol, atol): the project's values, and a loose pair
BLOCK = 256

C_SOL = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)
C_ERR = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
         -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1.0 / 60.0)
C_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
         187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


def fprod(a, b):
    """``a * b`` of two ``float`` scalars, as a kernel forms it."""
    return float(np.float32(a) * np.float32(b))


def per_row(vals, rpp, dtype):
    """One scalar per problem -> a (P rpp, 1) column."""
    return torch.tensor([float(v) for v in vals], dtype=dtype).repeat_interleave(rpp)[:, None]


# ---------------------------------------------------------------------------
# RK algebra
# ---------------------------------------------------------------------------
def affine_fwd(t):
    """f (n, n_s), g (n, n_s, n_u), u (n, n_u):  k = f + g u."""
    return dict(k=t["f"] + (t["g"] * t["u"][:, None, :]).sum(2))


def affine_bwd(t, mul=1.0, accumulate=False):
    """dg and du of sum(k * dk);  du = [du0 +] mul * d/du."""
    g = t["g"].clone().requires_grad_(True)
    u = t["u"].clone().requires_grad_(True)
    k = affine_fwd(dict(f=torch.zeros_like(t["dk"]), g=g, u=u))["k"]
    dg, du = torch.autograd.grad((k * t["dk"]).sum(), (g, u))
    du = f32(mul) * du
    return dict(dg=dg, du=t["du0"] + du if accumulate else du)


def rk_combine(t, coef, h, rpp):
    """out = (y0 or 0) + sum_j (coef_j h_p) K_j with K (n_k, n, n_s); a stage whose coefficient is 0 is skipped."""
    Ks = t["K"]
    a = t["y0"] if "y0" in t else torch.zeros_like(Ks[0])
    for j, c in enumerate(coef):
        if f32(c) != 0.0:
            a = a + Ks[j] * per_row([fprod(c, hp) for hp in h], rpp, Ks.dtype)
    return dict(out=a)


def live(coef):
    return [j for j, c in enumerate(coef) if f32(c) != 0.0]


def rk_stage_bwd(t, coef, h, rpp, n_s, n_ext=0, accumulate_dy0=False):
    """dY = dYup + dXf[:, :n_s] + dXg[:, :n_s];  dy0 (+)= dY;  dK_j += coef_j h dY;  du_ext += dXf[:, n_s:n_s+n_ext].
    ``dK`` holds the stages with a non-zero coefficient only (``live``): the others are not touched."""
    some = next(t[k] for k in ("dYup", "dXf", "dXg") if k in t)
    d = torch.zeros(some.shape[0], n_s, dtype=some.dtype)
    for k in ("dYup", "dXf", "dXg"):
        if k in t:
            d = d + t[k][:, :n_s]
    out = dict(dy0=t["dy0_0"] + d if accumulate_dy0 else d)
    if "dK0" in t:
        out["dK"] = torch.stack([t["dK0"][j] + per_row([fprod(coef[j], hp) for hp in h], rpp, d.dtype) * d
                                 for j in live(coef)])
    if n_ext:
        out["du_ext"] = t["du_ext0"] + t["dXf"][:, n_s:n_s + n_ext]
    return out


# ---------------------------------------------------------------------------
# norm sums
# ---------------------------------------------------------------------------
def _block_sums(q2, P, rpp):
    """q2 (P rpp, m) squares -> (P, nblk) sums over blocks of 256 rows.  float32: a row's columns first, then the rows
    one after the other; float64: torch's sum."""
    nblk = -(-rpp // BLOCK)
    rows = q2.sum(1).reshape(P, rpp)
    pad = torch.zeros(P, nblk * BLOCK, dtype=q2.dtype)
    pad[:, :rpp] = rows
    pad = pad.reshape(P, nblk, BLOCK)
    if q2.dtype == F64:
        return pad.sum(2)
    acc = torch.zeros(P, nblk, dtype=q2.dtype)
    for r in range(BLOCK):
        acc = acc + pad[:, :, r]
    return acc


def _scaled(mode, t, rtol, atol, y0key="y0", y1key="y1"):
    """The scaled quantities of one norm, squared: mode 0 -> (y0/scale, a/scale), mode 1 -> ((a - b)/scale,),
    mode 2 -> (a/tol,) with scale = atol + rtol |y0| and tol = atol + rtol max(|y0|, |y1|)."""
    rtol, atol = f32(rtol), f32(atol)
    y0 = t[y0key]
    if mode == 2:
        tol = atol + rtol * torch.maximum(y0.abs(), t[y1key].abs())
        return ((t["a"] / tol) ** 2,)
    sc = atol + y0.abs() * rtol
    if mode == 0:
        return (y0 / sc) ** 2, (t["a"] / sc) ** 2
    return (((t["a"] - t["b"]) / sc) ** 2,)


def _u_scaled(t, rtol, atol):
    u = t["u"]
    return (u / (f32(atol) + u.abs() * f32(rtol))) ** 2


def norm_sums(mode, t, rtol, atol, rpp, P):
    """partials (P, nblk, 2) of ``dopri_norm_block``.  mode 0: a = f0, u counts in column 0; mode 1: a = f1, b = f0;
    mode 2: a = err.  Column 1 is zero in modes 1 and 2."""
    q = _scaled(mode, t, rtol, atol)
    c0 = torch.cat((q[0], _u_scaled(t, rtol, atol)), 1) if mode == 0 else q[0]
    s0 = _block_sums(c0, P, rpp)
    s1 = _block_sums(q[1], P, rpp) if mode == 0 else torch.zeros_like(s0)
    return dict(partials=torch.stack((s0, s1), 2))


def adj_norm_sums(mode, t, rtol, atol, rpp, P, n_s):
    """partials (P, nblk, 4) of ``adj_norm_block`` on z = [y | a_x | a_u]: columns 0, 1 the y part (with u in mode 0's
    column 0), columns 2, 3 the [a_x | a_u] part."""
    q = _scaled(mode, t, rtol, atol, "Z0", "Z1")
    cols = []
    for part in (slice(0, n_s), slice(n_s, None)):
        c0 = q[0][:, part]
        if mode == 0 and part.start == 0:
            c0 = torch.cat((c0, _u_scaled(t, rtol, atol)), 1)
        s0 = _block_sums(c0, P, rpp)
        cols += [s0, _block_sums(q[1][:, part], P, rpp) if mode == 0 else torch.zeros_like(s0)]
    return dict(partials=torch.stack(cols, 2))


def rms_of(sums, rpp, n_cols):
    """sqrt(sum of a problem's block sums / (rpp n_cols)) in double, as the controllers form it.  sums: (nblk,)."""
    s = 0.0
    for v in np.asarray(sums, dtype=np.float64).reshape(-1):
        s += float(v)
    return float(np.sqrt(np.float64(s) / (float(rpp) * float(n_cols))))


# ---------------------------------------------------------------------------
# the controller
# ---------------------------------------------------------------------------
def _fmax(a, b):
    """C's fmax: the other operand where one is NaN."""
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return max(a, b)


def _fmin(a, b):
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return min(a, b)


def control(mode, n0, n1, c, t_end, n_slots=NO_SLOTS):
    """``dopri_control_vals`` on one problem's block ``c`` (16 floats); returns the new block.
    torchdiffeq's _select_initial_step / _compute_error_ratio / _optimal_step_size: safety 0.9, ifactor 10,
    dfactor 0.2; steps are not clipped to t_end."""
    c = list(c)
    if mode == 0:
        d0, d1 = n0, n1
        c[C_D0], c[C_D1] = d0, d1
        c[C_H0] = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        c[C_T] = c[C_NSTEPS] = c[C_DONE] = c[C_NACC] = c[C_OVF] = 0.0
    elif mode == 1:
        h0, d1 = c[C_H0], c[C_D1]
        d2 = n0 / h0
        c[C_D2] = d2
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(1e-6, h0 * 1e-3)
        else:
            h1 = (0.01 / _fmax(d1, d2)) ** (1.0 / 5.0)
        c[C_H] = _fmin(100.0 * h0, h1)
    else:
        ratio, h, t = n0, c[C_H], c[C_T]
        accept = ratio <= 1.0
        if ratio == 0.0:
            fac = 10.0
        else:
            dfac = 1.0 if ratio < 1.0 else 0.2
            fac = _fmin(10.0, _fmax(0.9 / ratio ** 0.2, dfac))
        c[C_RATIO], c[C_ACCEPT], c[C_HUSED] = ratio, (1.0 if accept else 0.0), h
        c[C_NSTEPS] += 1.0
        if accept and t + h >= t_end:
            c[C_DONE] = 1.0
            c[C_X] = (t_end - t) / h
        else:
            if accept:
                c[C_T] = t + h
                if int(c[C_NACC]) + 1 >= n_slots:
                    c[C_OVF] = c[C_DONE] = 1.0
                else:
                    c[C_NACC] += 1.0
            c[C_H] = h * fac
    return c


def control_launch(mode, n0, n1, c, t_end, n_slots=0, hslots=None, alog=None, alog_cap=0, skip_done=False):
    """One problem through a controller launch (``dopri_control_kernel`` and its fused / tile siblings): the machine
    above, the step-slot record ``hslots[slot_before] = h_try`` of an accepted attempt, and the attempt log's row
    ``n_steps - 1`` (nothing past ``alog_cap``).  ``skip_done``: the launch leaves a finished problem as it is.
    hslots: list (n_slots) or None; alog: list of [h, ratio, accept] rows or None.  Returns (c, hslots, alog)."""
    hslots = None if hslots is None else list(hslots)
    alog = None if alog is None else [list(r) for r in alog]
    if skip_done and mode == 2 and c[C_DONE] > 0.0:
        return list(c), hslots, alog
    slot_before, h_try = int(c[C_NACC]), c[C_H]
    c = control(mode, n0, n1, c, t_end, n_slots if n_slots > 0 else NO_SLOTS)
    if mode == 2:
        if hslots is not None and c[C_ACCEPT] > 0.0:
            hslots[slot_before] = h_try
        k = int(c[C_NSTEPS]) - 1
        if alog is not None and 0 <= k < alog_cap:
            alog[k] = [h_try, c[C_RATIO], c[C_ACCEPT]]
    return c, hslots, alog


def _max_keep_nan(a, b):
    """The larger of two norms, NaN if either is: a part that is not a number is not hidden behind a finite one."""
    return math.nan if (math.isnan(a) or math.isnan(b)) else max(a, b)


def adj_norms(s4, rpp, n_cols, pnorm=None):
    """(n0, n1) of ``adj_control_one``: the larger of the y part's and the adjoint part's RMS, and of ``pnorm`` (the
    parameter tensors' largest RMS, float32) where given; NaN if any of them is.  s4: a problem's four sums in double."""
    cnt = float(rpp) * float(n_cols)
    with np.errstate(invalid="ignore"):
        r = [float(np.sqrt(np.float64(v) / cnt)) for v in s4]
    n0, n1 = _max_keep_nan(r[0], r[2]), _max_keep_nan(r[1], r[3])
    if pnorm is not None:
        n0, n1 = _max_keep_nan(n0, float(pnorm[0])), _max_keep_nan(n1, float(pnorm[1]))
    return n0, n1


def adj_control(mode, s4, rpp, n_cols, pnorm, c, t_end):
    """``adj_control_kernel`` on one problem: a finished problem is left alone when an attempt is judged."""
    n0, n1 = adj_norms(s4, rpp, n_cols, pnorm)
    return control_launch(mode, n0, n1, c, t_end, skip_done=True)[0]


def ctl_block(seed=0, **fields):
    """A control block of distinct non-zero garbage with the named fields (``h=``, ``t=``, ``nacc=`` ...) set."""
    names = dict(h=C_H, t=C_T, ratio=C_RATIO, accept=C_ACCEPT, done=C_DONE, x=C_X, h0=C_H0, d0=C_D0, d1=C_D1, d2=C_D2,
                 nsteps=C_NSTEPS, hused=C_HUSED, nacc=C_NACC, ovf=C_OVF)
    c = [float(v) for v in (torch.rand(CTL, generator=gen(900 + seed), dtype=F64) * 7 + 3)]
    c[C_DONE] = c[C_OVF] = 0.0
    c[C_NSTEPS], c[C_NACC] = 5.0, 2.0
    for k, v in fields.items():
        c[names[k]] = float(v)
    return c


# ---------------------------------------------------------------------------
# the interpolant
# ---------------------------------------------------------------------------
USES = ("a", "b", "c")          # the polynomial's coefficients that read y0, y1 and y_mid


def per_use(t, keys, uses=USES):
    """``t`` with a copy ``key@use`` of each named tensor per use.  The interpolant reads y0, y1 and y_mid once per
    coefficient a, b, c, and the three cancel (at x = 1 the value is y1 whatever y0 and K are): with one copy per read
    the comparator perturbs each read on its own, so the bar follows the formula's sensitivity to a rounding of its
    terms and not only that of its value.  The copies are equal, so the reference is unchanged."""
    return dict(t, **{"%s@%s" % (k, u): t[k] for k in keys for u in uses})


def _use(t, k, u):
    return t.get("%s@%s" % (k, u), t[k])


def interp_poly(t, hv, ch):
    """torchdiffeq _interp_fit with the DPM mid-point coefficients: (a0, d, c, b, a) of
    y(t0 + x h) = a0 + x (d + x (c + x (b + x a))); hv: the (n, 1) column of h, ch[j]: that of cm_j * h."""
    co = {}
    for use in USES:
        y0, y1, Ks = (_use(t, k, use) for k in ("y0", "y1", "K"))
        ym = y0
        for j in range(7):
            if ch[j] is not None:
                ym = ym + Ks[j] * ch[j]
        f0, f1 = Ks[0], Ks[6]
        if use == "a":
            co[use] = 2 * hv * (f1 - f0) - 8 * (y1 + y0) + 16 * ym
        elif use == "b":
            co[use] = hv * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * ym
        else:
            co[use] = hv * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * ym
    return t["y0"], hv * t["K"][0], co["c"], co["b"], co["a"]


def _hx_columns(h, x, rpp, dt):
    ch = [per_row([fprod(cm, hp) for hp in h], rpp, dt) if f32(cm) != 0.0 else None for cm in C_MID]
    return per_row([f32(v) for v in h], rpp, dt), per_row([f32(v) for v in x], rpp, dt), ch


def interp(t, h, x, rpp, l=None):
    """y0, y1 (n, n_s), K (7, n, n_s); h, x: one float per problem.  out = y(t0 + x h) (_interp_evaluate); with ``l``
    the look-ahead point p = (out0 + l cos out2, out1 + l sin out2) too."""
    hv, xv, ch = _hx_columns(h, x, rpp, t["y0"].dtype)
    a0, d, c, b, a = interp_poly(t, hv, ch)
    out = a0 + xv * (d + xv * (c + xv * (b + xv * a)))
    res = dict(out=out)
    if l is not None:
        res["p"] = T.lookahead(dict(x=out), f32(l))["ps"]
    return res


def interp_bwd(t, h, x, rpp, l=None):
    """dy0, dy1, dK of sum(out * dout).  With ``l``: dout = d/dx sum(p(x) * (dps [+ dps2])) at x = ``xo``, the forward's
    output the backward launch is handed.  ``dout@1`` .. ``dout@4`` (``dps@k``, ``dps2@k``, ``xo@k``): the gradient as
    the term x^k reads it (``per_use``)."""
    src = "dout" if l is None else "dps"
    gs = []
    for k in range(5):
        g = _use(t, src, k) if k else t[src]
        if l is not None:
            q = dict(x=_use(t, "xo", k) if k else t["xo"], dps=g)
            if "dps2" in t:
                q["dps2"] = _use(t, "dps2", k) if k else t["dps2"]
            g = T.lookahead_bwd(q, f32(l))["dx"]
        gs.append(g)
    n, n_s = gs[0].shape
    dt = gs[0].dtype
    v = [torch.zeros(n, n_s, dtype=dt, requires_grad=True), torch.zeros(n, n_s, dtype=dt, requires_grad=True),
         torch.zeros(7, n, n_s, dtype=dt, requires_grad=True)]
    hv, xv, ch = _hx_columns(h, x, rpp, dt)
    co = interp_poly(dict(y0=v[0], y1=v[1], K=v[2]), hv, ch)
    L = sum((c * g * xv ** k).sum() for k, (c, g) in enumerate(zip(co, gs)))
    dy0, dy1, dK = torch.autograd.grad(L, v)
    return dict(dy0=dy0, dy1=dy1, dK=dK)


GRAD_USES = (1, 2, 3, 4)          # the terms x^1 .. x^4 of the backward


# ---------------------------------------------------------------------------
# adjoint glue
# ---------------------------------------------------------------------------
def param_norm(mode, t, segs, h, rtol, atol, c_sol=C_SOL, c_err=C_ERR):
    """th0 (N), K (S, N); segs: [(offset, length)].  Per tensor the RMS of the scaled quantity, pnorm = the largest
    (column 1: mode 0 only).  mode 2 also: th1 = th0 + h sum c_sol_j K_j on the segments (concatenated)."""
    th0, Ks = t["th0"], t["K"]
    dt = th0.dtype
    rtol, atol = f32(rtol), f32(atol)
    m = [torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)]
    th1s = []
    for off, ln in segs:
        z0 = th0[off:off + ln]
        sc = atol + z0.abs() * rtol
        if mode == 0:
            qs = [(z0 / sc) ** 2, (Ks[0, off:off + ln] / sc) ** 2]
        elif mode == 1:
            qs = [((Ks[1, off:off + ln] - Ks[0, off:off + ln]) / sc) ** 2]
        else:
            z1, er = z0, torch.zeros_like(z0)
            for j in range(Ks.shape[0]):
                k = Ks[j, off:off + ln]
                if f32(c_sol[j]) != 0.0:
                    z1 = z1 + k * fprod(c_sol[j], h)
                if f32(c_err[j]) != 0.0:
                    er = er + k * fprod(c_err[j], h)
            th1s.append(z1)
            qs = [(er / (atol + rtol * torch.maximum(z0.abs(), z1.abs()))) ** 2]
        for col, q in enumerate(qs):
            if dt == F64:
                s = q.sum()
            else:
                s = torch.zeros((), dtype=dt)
                for v in q:
                    s = s + v
            m[col] = torch.maximum(m[col], s / torch.tensor(float(ln), dtype=dt))
    out = dict(pnorm=torch.sqrt(torch.stack(m)))
    if mode == 2:
        out["th1"] = torch.cat(th1s)
    return out


def commit(ctl, rpp, dst, src):
    """Rows of problems with accept > 0 and done == 0 take the source rows; all other rows stay."""
    out = dst.clone()
    for p in range(dst.shape[0] // rpp):
        c = ctl[p]
        if c[C_ACCEPT] > 0.0 and not c[C_DONE] > 0.0:
            out[p * rpp:(p + 1) * rpp] = src[p * rpp:(p + 1) * rpp]
    return out


def pack(y, a_x, n_u):
    """z = [y | a_x | a_u = 0]."""
    return torch.cat((y, a_x, torch.zeros(y.shape[0], n_u, dtype=y.dtype)), 1)


def unpack(Z, n_s, n_u):
    """(dy0, du) = (a_x, a_u) of z."""
    return Z[:, n_s:2 * n_s].clone(), Z[:, 2 * n_s:2 * n_s + n_u].clone()


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def reference_and_bar(op, fn, inputs):
    return T.reference_and_bar(op, fn, inputs, k=K[op])


bar_ratio = T.bar_ratio


# ---------------------------------------------------------------------------
# shared cases (float32 tensors; built once, read unchanged)
# ---------------------------------------------------------------------------
SHARED = tuple((rows, P, n_s, n_u, 0) for rows in ROWS for P in (1, 3) for (n_s, n_u) in DIMS) + (
    (257, 8, 6, 2, 0), (600, 3, 6, 2, 1))
H_CYCLE = (0.05, 0.7, 1e-4)          # the step per problem
X_CYCLE = (0.37, 1.0, 1e-6, 0.0)     # the interpolation abscissa: problem p of shared case i reads X_CYCLE[(i + p) % 4]
ERR_SCALE = (0.5, 1.9, 0.7)            # per problem: the error's size in units of the tolerance


def key_label(key):
    return "rows%d P%d ns%d nu%d tol%d" % key


def _mags(g, w):
    return torch.tensor(MAGS)[torch.randint(0, 3, (w,), generator=g)]


@functools.lru_cache(maxsize=None)
def state_case(rows, P, n_s, n_u, tol=0):
    """One solve's per-row tensors: y0 (every seventh row exactly zero), y1, f0, f1, err (ERR_SCALE tolerances large per
    problem), u, K (7 stages); column magnitudes drawn from MAGS."""
    rtol, atol = TOLS[tol]
    g = gen(5000 + rows * 131 + P * 17 + n_s * 7 + n_u + 1000 * tol)
    n = P * rows
    ms, mu = _mags(g, n_s), _mags(g, n_u)
    y0 = randn(g, n, n_s) * ms
    y0[::7] = 0.0
    f0 = randn(g, n, n_s) * ms
    f1 = f0 + 0.1 * randn(g, n, n_s) * ms
    Ks = randn(g, 7, n, n_s) * ms
    Ks[0], Ks[6] = f0, f1
    h = [H_CYCLE[p % 3] for p in range(P)]
    y1 = rk_combine(dict(y0=y0, K=Ks), C_SOL, h, rows)["out"]          # a step's own result
    tolv = atol + rtol * torch.maximum(y0.abs(), y1.abs())
    scale = torch.tensor([ERR_SCALE[p % 3] for p in range(P)]).repeat_interleave(rows)[:, None]
    return types.SimpleNamespace(rows=rows, P=P, n_s=n_s, n_u=n_u, n=n, rtol=rtol, atol=atol, y0=y0, y1=y1, f0=f0, f1=f1,
                                 err=randn(g, n, n_s) * tolv * scale, u=randn(g, n, n_u) * mu,
                                 K=Ks, h=h)


@functools.lru_cache(maxsize=None)
def adj_case(rows, P, n_s, n_u, tol=0):
    """The augmented state z = [y | a_x | a_u] (a_u non-zero), its step result, two stage derivatives and an error."""
    rtol, atol = TOLS[tol]
    g = gen(7000 + rows * 131 + P * 17 + n_s * 7 + n_u + 1000 * tol)
    n, W = P * rows, 2 * n_s + n_u
    mz = _mags(g, W)
    Z0 = randn(g, n, W) * mz
    Z0[::7] = 0.0
    Z1 = Z0 + 0.05 * randn(g, n, W) * mz
    a = randn(g, n, W) * mz
    tolv = atol + rtol * torch.maximum(Z0.abs(), Z1.abs())
    scale = torch.tensor([ERR_SCALE[p % 3] for p in range(P)]).repeat_interleave(rows)[:, None]
    return types.SimpleNamespace(rows=rows, P=P, n_s=n_s, n_u=n_u, n=n, W=W, rtol=rtol, atol=atol, Z0=Z0, Z1=Z1, a=a,
                                 b=a + 0.1 * randn(g, n, W) * mz, err=randn(g, n, W) * tolv * scale,
                                 u=randn(g, n, n_u) * _mags(g, n_u))


def norm_inputs(mode, s):
    """The tensors ``norm_sums`` reads in ``mode`` out of a state case."""
    if mode == 0:
        return dict(y0=s.y0, a=s.f0, u=s.u)
    if mode == 1:
        return dict(y0=s.y0, a=s.f1, b=s.f0)
    return dict(y0=s.y0, y1=s.y1, a=s.err)


def adj_norm_inputs(mode, s):
    if mode == 0:
        return dict(Z0=s.Z0, a=s.a, u=s.u)
    if mode == 1:
        return dict(Z0=s.Z0, a=s.b, b=s.a)
    return dict(Z0=s.Z0, Z1=s.Z1, a=s.err)


def case(op, label, fn, inputs, **meta):
    return types.SimpleNamespace(op=op, label=label, fn=fn, inputs=inputs, meta=types.SimpleNamespace(**meta))


@functools.lru_cache(maxsize=None)
def norm_cases():
    out = []
    for key in SHARED:
        s = state_case(*key)
        for mode in (0, 1, 2):
            out.append(case("norm_sums%d" % mode, key_label(key),
                            functools.partial(norm_sums, mode, rtol=s.rtol, atol=s.atol, rpp=s.rows, P=s.P),
                            norm_inputs(mode, s), key=key, mode=mode))
    return out


@functools.lru_cache(maxsize=None)
def adj_norm_cases():
    out = []
    for key in SHARED:
        s = adj_case(*key)
        for mode in (0, 1, 2):
            out.append(case("adj_norm_sums%d" % mode, key_label(key),
                            functools.partial(adj_norm_sums, mode, rtol=s.rtol, atol=s.atol, rpp=s.rows, P=s.P, n_s=s.n_s),
                            adj_norm_inputs(mode, s), key=key, mode=mode))
    return out


@functools.lru_cache(maxsize=None)
def affine_cases():
    """n rows of (f, g, u, dk): forward, and the backward with dg NULL / given, du NULL / overwritten / accumulated
    onto a non-zero buffer, mul 1 and -0.375."""
    out = []
    for n in ROWS:
        for (n_s, n_u) in DIMS[:3]:
            g = gen(6000 + n * 31 + n_s)
            f, gg, u = randn(g, n, n_s) * _mags(g, n_s), randn(g, n, n_s, n_u), randn(g, n, n_u) * _mags(g, n_u)
            lab = "n%d ns%d nu%d" % (n, n_s, n_u)
            out.append(case("affine_fwd", lab, affine_fwd, dict(f=f, g=gg, u=u), n=n, n_s=n_s, n_u=n_u))
            dk, du0 = randn(g, n, n_s), randn(g, n, n_u) * 10
            for want_dg, du_mode, mul in ((True, "overwrite", 1.0), (False, "accumulate", -0.375), (True, "null", 1.0),
                                          (True, "accumulate", 2.5)):
                t = dict(dk=dk, g=gg, u=u)
                if du_mode == "accumulate":
                    t["du0"] = du0
                out.append(case("affine_bwd", "%s dg%d du-%s mul%g" % (lab, want_dg, du_mode, mul),
                                functools.partial(affine_bwd, mul=mul, accumulate=du_mode == "accumulate"), t,
                                n=n, n_s=n_s, n_u=n_u, want_dg=want_dg, du_mode=du_mode, mul=mul))
    return out


COEF4 = (0.25, -1.5, 0.0, 0.8125)


@functools.lru_cache(maxsize=None)
def rk_combine_cases():
    """Per shared case: (y0 given, h by value, the seven dopri5 c_sol coefficients: the two zero ones point at stages
    filled with NaN) and (y0 NULL, h read from a control block, four stages)."""
    out = []
    for key in SHARED:
        s = state_case(*key)
        K7 = s.K.clone()
        K7[1], K7[6] = float("nan"), float("nan")
        out.append(case("rk_combine", key_label(key) + " y0 h_host c_sol",
                        functools.partial(rk_combine, coef=C_SOL, h=s.h, rpp=s.rows), dict(y0=s.y0, K=K7),
                        key=key, coef=C_SOL, y0=True, h_dev=False))
        K4 = s.K[:4].clone()
        K4[2] = float("nan")
        out.append(case("rk_combine", key_label(key) + " no-y0 h_dev",
                        functools.partial(rk_combine, coef=COEF4, h=s.h, rpp=s.rows), dict(K=K4),
                        key=key, coef=COEF4, y0=False, h_dev=True))
    return out


STAGE_KEYS = tuple(k for k in SHARED if k[1] in (1, 3) and k[2] != 8)


@functools.lru_cache(maxsize=None)
def rk_stage_bwd_cases():
    """The drivers' forms: the solution row (dYup alone, dy0 overwritten), an affine stage (dYup + dXf + dXg, or the two
    input gradients alone, dy0 accumulated), a single-net stage (dYup + dXf with the carried inputs' columns into
    du_ext), dy0 NULL; dx_ld = n_s + n_ext + 3; dK accumulates onto non-zero contents and the stage behind the zero
    coefficient is NaN."""
    out = []
    forms = ((("dYup",), "overwrite", 0, False), (("dYup", "dXf", "dXg"), "accumulate", 0, True),
             (("dXf", "dXg"), "accumulate", 0, False), (("dYup", "dXf"), "accumulate", 2, True),
             (("dXf",), "null", 2, False))
    for i, key in enumerate(STAGE_KEYS):
        s = state_case(*key)
        g = gen(8000 + i)
        for srcs, dy0_mode, n_ext, h_dev in forms:
            ld = s.n_s + n_ext + 3
            t = {k: (randn(g, s.n, s.n_s) if k == "dYup" else randn(g, s.n, ld)) for k in srcs}
            dK0 = randn(g, 4, s.n, s.n_s)
            dK0[2] = float("nan")
            t["dK0"] = dK0
            if dy0_mode == "accumulate":
                t["dy0_0"] = randn(g, s.n, s.n_s) * 3
            if n_ext:
                t["du_ext0"] = randn(g, s.n, n_ext)
            out.append(case("rk_stage_bwd", "%s %s dy0-%s ext%d" % (key_label(key), "+".join(srcs), dy0_mode, n_ext),
                            functools.partial(rk_stage_bwd, coef=COEF4, h=s.h, rpp=s.rows, n_s=s.n_s, n_ext=n_ext,
                                              accumulate_dy0=dy0_mode == "accumulate"), t,
                            key=key, srcs=srcs, dy0_mode=dy0_mode, n_ext=n_ext, ld=ld, h_dev=h_dev))
    return out


L_P = T.L_P


@functools.lru_cache(maxsize=None)
def interp_cases():
    """Per shared case the forward and the backward at the case's steps (y1 is that step's result) and abscissae
    walking X_CYCLE: every (h, x) pair occurs; n_s == 3 cases also with the look-ahead map (backward with and
    without dp2)."""
    out = []
    for i, key in enumerate(SHARED):
        s = state_case(*key)
        g = gen(9000 + i)
        h, x = s.h, [X_CYCLE[(i + p) % 4] for p in range(s.P)]
        lab = key_label(key) + " x%g" % x[0]
        t = per_use(dict(y0=s.y0, y1=s.y1, K=s.K), ("y0", "y1", "K"))
        out.append(case("interp", lab, functools.partial(interp, h=h, x=x, rpp=s.rows), t, key=key, h=h, x=x, l=None))
        out.append(case("interp_bwd", lab, functools.partial(interp_bwd, h=h, x=x, rpp=s.rows),
                        per_use(dict(dout=randn(g, s.n, s.n_s)), ("dout",), GRAD_USES), key=key, h=h, x=x, l=None))
        if s.n_s == 3:
            t3 = per_use(dict(y0=s.y0 * 0.125, y1=s.y1 * 0.125, K=s.K * 0.125), ("y0", "y1", "K"))
            out.append(case("interp_map", lab, functools.partial(interp, h=h, x=x, rpp=s.rows, l=L_P), t3,
                            key=key, h=h, x=x, l=L_P))
            xo = T.run(functools.partial(interp, h=h, x=x, rpp=s.rows), t3, F64)["out"].float()
            for two in (False, True):
                tb = dict(dps=randn(g, s.n, 2), xo=xo)
                if two:
                    tb["dps2"] = randn(g, s.n, 2)
                tb = per_use(tb, tuple(tb), GRAD_USES)
                out.append(case("interp_map_bwd", lab + " dp2=%d" % two,
                                functools.partial(interp_bwd, h=h, x=x, rpp=s.rows, l=L_P), tb, key=key, h=h, x=x, l=L_P))
    return out


SEG_LENS = (1, 255, 257, 1000)
SEG_GAP = 5


def segments():
    """[(offset, length)] of SEG_LENS laid out with gaps of SEG_GAP floats, and the total length."""
    segs, off = [], 3
    for ln in SEG_LENS:
        segs.append((off, ln))
        off += ln + SEG_GAP
    return segs, off


@functools.lru_cache(maxsize=None)
def param_cases():
    """Modes 0 / 1 / 2 on the segments; ``big`` names the segment that holds the largest RMS (the length-1 one, or the
    longest)."""
    segs, N = segments()
    out = []
    for big in (0, 3):
        g = gen(9500 + big)
        th0 = randn(g, N) * 0.3
        Ks = randn(g, 7, N) * 0.1
        off, ln = segs[big]
        Ks[:, off:off + ln] *= 40.0          # (th0 / scale sits near 1 / rtol in every tensor; the K terms do not)
        for mode in (0, 1, 2):
            out.append(case("param_norm%d" % mode, "big%d" % big,
                            functools.partial(param_norm, mode, segs=segs, h=0.05, rtol=TOLS[0][0], atol=TOLS[0][1]),
                            dict(th0=th0, K=Ks), big=big, mode=mode, h=0.05))
    return out


def all_cases():
    return (affine_cases() + rk_combine_cases() + rk_stage_bwd_cases() + norm_cases() + adj_norm_cases()
            + interp_cases() + param_cases())


# ---------------------------------------------------------------------------
# controller cases on hand-made partials
# ---------------------------------------------------------------------------
def partial_for(ratio, cnt):
    """A float32 sum s with sqrt(s / cnt) ~ ratio (exactly, where ratio^2 cnt is a float32)."""
    return float(np.float32(np.float64(ratio) ** 2 * cnt))


# ---------------------------------------------------------------------------
# fused norm + control launches on the shared cases
# ---------------------------------------------------------------------------
FUSED_T_END = 0.8
FUSED_T = (0.78, 0.2, 0.5)       # with H_CYCLE and ERR_SCALE: problem 0 finishes, 1 is rejected, 2 is accepted and goes on


def _f64_norms(key, mode, adjoint):
    """[(n0, n1)] per problem from the float64 sums."""
    s = adj_case(*key) if adjoint else state_case(*key)
    if adjoint:
        part = T.run(functools.partial(adj_norm_sums, mode, rtol=s.rtol, atol=s.atol, rpp=s.rows, P=s.P, n_s=s.n_s),
                     adj_norm_inputs(mode, s), F64)["partials"]
        return [adj_norms([float(v) for v in part[p].sum(0)], s.rows, s.n_s + s.n_u) for p in range(s.P)]
    part = T.run(functools.partial(norm_sums, mode, rtol=s.rtol, atol=s.atol, rpp=s.rows, P=s.P),
                 norm_inputs(mode, s), F64)["partials"]
    return [(rms_of(part[p, :, 0], s.rows, s.n_s + s.n_u), rms_of(part[p, :, 1], s.rows, s.n_s + s.n_u))
            for p in range(s.P)]


@functools.lru_cache(maxsize=None)
def fused_reference(key, mode, adjoint):
    """Per problem (the control block a fused launch of ``mode`` is handed, n0, n1 of the float64 sums).  The block is
    what the reference's earlier modes leave; before mode 2 the step is the case's own (y1 is its result), the time
    FUSED_T and the step counters small non-zero numbers."""
    s = state_case(*key)
    out = []
    norms = {m: _f64_norms(key, m, adjoint) for m in range(mode + 1)}
    for p in range(s.P):
        c = ctl_block(10 + p)
        if mode >= 1:
            c = control(0, norms[0][p][0], norms[0][p][1], c, FUSED_T_END)
        if mode == 2:
            c = control(1, norms[1][p][0], 0.0, c, FUSED_T_END)
            c[C_H], c[C_T], c[C_NACC], c[C_NSTEPS] = s.h[p], FUSED_T[p % 3], float(p % 3), float(p)
        out.append((c, norms[mode][p][0], norms[mode][p][1]))
    return out
