"""The references and bars of ``ode_control_common`` are themselves checked, on the CPU: the controller, the norm sums
and the interpolant re-walk float64 solves of the oracle (``oracle/nlbac_oracle.py``) and must reproduce its initial
step, its attempt sequence and its result; the float32 evaluation of every reference stays within half its bar on every
case (the condition that fixes ``K``); and the shared cases keep clear of the controller's branch points, so that a
float32 summation order cannot flip a branch on the device.

The oracle takes its tolerances as doubles and the references round theirs to float32, as the ABI does: the anchors use
rtol = 2^-17 and atol = 2^-23, which are both."""
import math

import numpy as np
import pytest
import torch

import ode_control_common as Q
import task_kernels_common as T
from oracle import nlbac_oracle as O

F32, F64 = torch.float32, torch.float64
RTOL, ATOL = 2.0 ** -17, 2.0 ** -23
N_S, N_U, ROWS = 3, 2, 300          # two blocks per problem, the second ragged


def close(a, b, tol=1e-12):
    return abs(a - b) <= tol * abs(b)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


class Field:
    """dx/dt = x A^T + u B^T on rows [x | u]; the action columns are carried with zero derivative."""

    def __init__(self, eig, seed):
        g = T.gen(seed)
        q, _ = torch.linalg.qr(torch.randn(N_S, N_S, generator=g, dtype=F64))
        self.A = q @ torch.diag(torch.tensor(eig, dtype=F64)) @ q.T
        self.B = torch.randn(N_S, N_U, generator=g, dtype=F64)
        self.y0 = torch.randn(ROWS, N_S + N_U, generator=g, dtype=F64)
        self.y0[::7, :N_S] = 0.0

    def __call__(self, t, y):
        x, u = y[:, :N_S], y[:, N_S:]
        return torch.cat((x @ self.A.T + u @ self.B.T, torch.zeros_like(u)), 1)


FIELDS = {"stable": ((-0.5, -1.0, -2.0), 1.0), "stiff": ((-1.0, -40.0, -900.0), 1.0)}


def norm_of(mode, t):
    """The RMS norm the controller is fed: ``norm_sums`` in float64, summed over the blocks."""
    s = Q.norm_sums(mode, t, RTOL, ATOL, ROWS, 1)["partials"][0]
    return Q.rms_of(s[:, 0], ROWS, N_S + N_U), Q.rms_of(s[:, 1], ROWS, N_S + N_U)


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_controller_reproduces_the_oracles_solve(name):
    eig, t_end = FIELDS[name]
    func = Field(eig, 11)
    y0 = func.y0
    info = {}
    want = O.odeint(func, y0, [0.0, t_end], "dopri5", atol=ATOL, rtol=RTOL, info=info)[1]
    steps = info["steps"]
    f0 = func(0.0, y0)
    h_want = O.dopri5_initial_step(func, 0.0, y0, f0, RTOL, ATOL)

    X = lambda y: y[:, :N_S]
    c = Q.ctl_block(1)
    c = Q.control(0, *norm_of(0, dict(y0=X(y0), a=X(f0), u=y0[:, N_S:])), c, t_end)
    assert c[Q.C_T] == 0.0 and c[Q.C_NSTEPS] == 0.0 and c[Q.C_DONE] == 0.0 and c[Q.C_NACC] == 0.0
    f1 = func(c[Q.C_H0], y0 + np.float32(c[Q.C_H0]) * f0)
    c = Q.control(1, norm_of(1, dict(y0=X(y0), a=X(f1), b=X(f0)))[0], 0.0, c, t_end)
    print("%s: initial step %.17g, the oracle's %.17g" % (name, c[Q.C_H], h_want))
    assert close(c[Q.C_H], h_want)

    tc, yc, fc, out = 0.0, y0, f0, None
    for i, (h_o, ratio_o, accept_o) in enumerate(steps):
        h = c[Q.C_H]
        yn, fn, err, k = O.dopri5_step(func, tc, h, yc, fc)
        ratio = norm_of(2, dict(y0=X(yc), y1=X(yn), a=X(err)))[0]
        c = Q.control(2, ratio, 0.0, c, t_end)
        assert close(h, h_o) and close(ratio, ratio_o, 1e-10) and (c[Q.C_ACCEPT] > 0) == bool(accept_o), (i, h, h_o)
        assert c[Q.C_HUSED] == h and c[Q.C_NSTEPS] == i + 1
        if c[Q.C_DONE] > 0:
            assert i == len(steps) - 1
            out = Q.interp(dict(y0=yc, y1=yn, K=torch.stack(k)), [h], [c[Q.C_X]], ROWS)["out"]
            break
        if c[Q.C_ACCEPT] > 0:
            tc, yc, fc = c[Q.C_T], yn, fn
    n_rej = sum(1 for s in steps if not s[2])
    print("%s: %d attempts, %d rejected" % (name, len(steps), n_rej))
    if name == "stiff":
        assert n_rej >= 1
    assert out is not None and rel(out, want) <= 1e-12
    assert c[Q.C_NACC] == sum(1 for s in steps if s[2]) - 1 and c[Q.C_OVF] == 0.0


def test_adjoint_controller_reproduces_the_oracles_tuple_solve():
    """z = ([y | u], [a_x | a_u], theta_0 (3), theta_1 (1)): the mixed norm is the largest of the parts' RMS norms, every
    parameter tensor on its own (``adj_norm_sums`` + ``param_norm`` -> ``adj_norms``)."""
    g = T.gen(5)
    n, m, t_end = ROWS, N_S + N_U, 1.0
    M = torch.randn(m, m, generator=g, dtype=F64) * 0.7
    M[N_S:] = 0.0                                            # the carried controls have zero derivative
    z0 = [torch.randn(n, m, generator=g, dtype=F64), torch.randn(n, m, generator=g, dtype=F64) * 30,
          torch.randn(3, generator=g, dtype=F64) * 0.1, torch.tensor([25.0], dtype=F64)]
    segs = [(0, 3), (5, 1)]

    def G(z):
        return [z[0] @ M.T, -(z[1] @ M), -0.5 * z[2] + 0.1 * z[1].mean(), 2.0 * z[3]]

    info = {}
    want = O.odeint_tuple(G, z0, t_end, "dopri5", ATOL, RTOL, info)
    steps = info["steps"]

    def Z(z):        # [y | a_x | a_u] and u
        return torch.cat((z[0][:, :N_S], z[1]), 1), z[0][:, N_S:]

    def flat(z):
        th = torch.zeros(6, dtype=F64)
        th[0:3], th[5:6] = z[2], z[3]
        return th

    def norms(mode, rows, par):
        s = Q.adj_norm_sums(mode, rows, RTOL, ATOL, n, 1, N_S)["partials"][0].sum(0)
        pn = Q.param_norm(mode, par, segs, par.pop("h", 0.0), RTOL, ATOL)["pnorm"]
        return Q.adj_norms([float(v) for v in s], n, m, [float(v) for v in pn])

    f0 = G(z0)
    c = Q.ctl_block(2)
    Z0, u = Z(z0)
    c = Q.control(0, *norms(0, dict(Z0=Z0, a=Z(f0)[0], u=u), dict(th0=flat(z0), K=flat(f0)[None])), c, t_end)
    f1 = G(O._tuple_axpy(z0, [f0], [1.0], np.float32(c[Q.C_H0])))
    c = Q.control(1, norms(1, dict(Z0=Z0, a=Z(f1)[0], b=Z(f0)[0]),
                           dict(th0=flat(z0), K=torch.stack((flat(f0), flat(f1)))))[0], 0.0, c, t_end)
    assert close(c[Q.C_H], steps[0][0])
    zc, fc, out, dominated = z0, f0, None, 0
    for i, (h_o, ratio_o, accept_o) in enumerate(steps):
        h = c[Q.C_H]
        hf = np.float32(h)
        ks = [fc]
        for beta in O._DP_BETA:
            zi = O._tuple_axpy(zc, ks, beta, hf)
            ks.append(G(zi))
        err = [sum(k[j] * (np.float32(cc) * hf) for cc, k in zip(O._DP_C_ERR, ks)) for j in range(4)]
        par = dict(th0=flat(zc), K=torch.stack([flat(k) for k in ks]), h=h)
        th1 = Q.param_norm(2, dict(par), segs, h, RTOL, ATOL)["th1"]
        assert rel(th1, torch.cat((zi[2], zi[3]))) <= 1e-14
        n0, _ = norms(2, dict(Z0=Z(zc)[0], Z1=Z(zi)[0], a=Z(err)[0]), par)
        rows_only = Q.adj_norms([float(v) for v in Q.adj_norm_sums(2, dict(Z0=Z(zc)[0], Z1=Z(zi)[0], a=Z(err)[0]), RTOL,
                                                                   ATOL, n, 1, N_S)["partials"][0].sum(0)], n, m)[0]
        dominated += n0 > rows_only
        c = Q.control(2, n0, 0.0, c, t_end)
        assert close(h, h_o) and close(n0, ratio_o, 1e-10) and (c[Q.C_ACCEPT] > 0) == bool(accept_o), (i, h, h_o)
        if c[Q.C_DONE] > 0:
            out = [Q.interp(dict(y0=zc[j].reshape(1, -1), y1=zi[j].reshape(1, -1),
                                 K=torch.stack([k[j].reshape(1, -1) for k in ks])), [h], [c[Q.C_X]], 1)["out"]
                   for j in range(4)]
            break
        if c[Q.C_ACCEPT] > 0:
            zc, fc = zi, ks[-1]
    print("adjoint: %d attempts, %d rejected, the parameter norm led in %d" % (
        len(steps), sum(1 for s in steps if not s[2]), dominated))
    assert dominated >= 1, "the parameter tensors never led the norm: the case does not exercise pnorm"
    assert out is not None
    for j in range(4):
        assert rel(out[j].reshape(-1), want[j].reshape(-1)) <= 1e-12


def test_interpolant_is_the_oracles():
    s = Q.state_case(257, 3, 6, 2)
    t = dict(y0=s.y0.double(), y1=s.y1.double(), K=s.K.double())
    for p, h in enumerate(s.h):
        rows = slice(p * s.rows, (p + 1) * s.rows)
        tp = dict(y0=t["y0"][rows], y1=t["y1"][rows], K=t["K"][:, rows])
        for x in (0.0, 1e-6, 0.37, 1.0):
            got = Q.interp(tp, [h], [x], s.rows)["out"]
            want = O.dopri5_interp(tp["y0"], tp["y1"], list(tp["K"]), h, x)
            assert rel(got, want) <= 1e-13, (h, x)
            if x == 0.0:
                assert torch.equal(got, tp["y0"])
    inputs = Q.per_use(dict(y0=s.y0, y1=s.y1, K=s.K), ("y0", "y1", "K"))
    ref, bar = Q.reference_and_bar("interp", lambda q: Q.interp(q, s.h, [1.0] * s.P, s.rows), inputs)
    r = Q.bar_ratio(s.y1.double().numpy(), ref["out"], bar["out"])
    print("interp(x = 1) against y1: %.3f of the bar" % r)
    assert r <= 1.0


def test_interp_backward_is_the_adjoint_of_the_forward():
    """<g, fwd(v)> == <bwd(g), v> in float64: the forward is linear in v = (y0, y1, K)."""
    s = Q.state_case(255, 3, 3, 2)
    g = torch.randn(s.n, s.n_s, generator=T.gen(3), dtype=F64)
    x = [0.37, 1.0, 1e-6]
    v = dict(y0=s.y0.double(), y1=s.y1.double(), K=s.K.double())
    lhs = (Q.interp(v, s.h, x, s.rows)["out"] * g).sum()
    b = Q.interp_bwd(dict(dout=g), s.h, x, s.rows)
    rhs = (b["dy0"] * v["y0"]).sum() + (b["dy1"] * v["y1"]).sum() + (b["dK"] * v["K"]).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))


def test_float32_reference_within_half_the_bar():
    """The condition that fixes K: on every case the float32 evaluation of the reference is within half the bar, and no
    smaller power of two would do."""
    worst = {}
    for c in Q.all_cases():
        ref, bar = Q.reference_and_bar(c.op, c.fn, c.inputs)
        lo = T.run(c.fn, c.inputs, F32)
        assert set(lo) == set(ref)
        r = max(Q.bar_ratio(lo[k].double().numpy(), ref[k], bar[k]) for k in ref)
        if r >= worst.get(c.op, (-1.0, ""))[0]:
            worst[c.op] = (r, c.label)
    assert set(worst) == set(Q.K)
    for op in Q.K:
        print("float32 reference / bar  %-16s K %-3d %.3f   (%s)" % (op, Q.K[op], worst[op][0], worst[op][1]))
    for op in Q.K:
        assert worst[op][0] <= 0.5, "%s: the float32 reference is at %.3f of the bar (%s)" % ((op,) + worst[op])
        assert Q.K[op] == 1 or worst[op][0] > 0.25, "%s: K = %d is not the smallest power of two" % (op, Q.K[op])


def test_shared_cases_are_what_they_claim():
    for key in Q.SHARED:
        s = Q.state_case(*key)
        assert bool((s.y0[::7] == 0).all()) and bool((s.y0[1::7] != 0).all())
        assert bool(torch.equal(s.y1, Q.rk_combine(dict(y0=s.y0, K=s.K), Q.C_SOL, s.h, s.rows)["out"]))
        a = Q.adj_case(*key)
        assert bool((a.Z0[:, 2 * a.n_s:] != 0).any()) or a.n_u == 0 or a.rows == 1      # (row 0 is a zero row)
    assert {k[0] for k in Q.SHARED} == set(Q.ROWS) and {k[1] for k in Q.SHARED} == {1, 3, 8}
    assert {(k[2], k[3]) for k in Q.SHARED} == set(Q.DIMS) and {k[4] for k in Q.SHARED} == {0, 1}
    for s_ in (Q.state_case(600, 3, 6, 2), Q.state_case(600, 3, 6, 2, 1)):
        assert (s_.rtol, s_.atol) in Q.TOLS
    pairs = {(h, x) for c in Q.interp_cases() for h, x in zip(c.meta.h, c.meta.x)}
    assert pairs == {(h, x) for h in Q.H_CYCLE for x in Q.X_CYCLE}
    segs, N = Q.segments()
    assert [ln for _, ln in segs] == list(Q.SEG_LENS) and all(b[0] - (a[0] + a[1]) == Q.SEG_GAP for a, b in zip(segs, segs[1:]))
    for c in Q.param_cases():          # the named segment leads the maximum
        for col in range(2 if c.meta.mode == 0 else 1):
            per = [float(Q.param_norm(c.meta.mode, T.run(lambda q: q, c.inputs, F64), [sg], c.meta.h, *Q.TOLS[0])["pnorm"][col])
                   for sg in segs]
            lead = int(np.argmax(per))
            print("param_norm%d big%d col%d: per-tensor RMS %s" % (c.meta.mode, c.meta.big, col, ["%.3g" % v for v in per]))
            if not (c.meta.mode == 0 and col == 0):      # (th0 / scale sits at 1 / rtol in every tensor)
                assert lead == c.meta.big


def test_shared_cases_keep_clear_of_the_branch_points():
    """A condition on the inputs: every row-derived norm that a fused norm + control launch feeds into the controller is
    far enough from the controller's comparisons that no float32 summation order can change the branch."""
    for key in Q.SHARED:
        for adjoint in (False, True):
            for mode in (0, 1, 2):
                for p, (c, n0, n1) in enumerate(Q.fused_reference(key, mode, adjoint)):
                    lab = "%s adjoint%d mode%d problem%d" % (Q.key_label(key), adjoint, mode, p)
                    if mode == 0:
                        for d in (n0, n1):
                            assert d < 0.5e-5 or d > 2e-5, lab
                    elif mode == 1:
                        d1, d2, h0 = c[Q.C_D1], n0 / c[Q.C_H0], c[Q.C_H0]
                        assert max(d1, d2) > 1e-12, lab
                        cap = 100.0 * h0 / (0.01 / max(d1, d2)) ** 0.2
                        assert abs(cap - 1.0) > 1e-3, lab
                    else:
                        assert abs(n0 - 1.0) > 1e-3, "%s: ratio %.6f" % (lab, n0)
                        assert abs(c[Q.C_T] + c[Q.C_H] - Q.FUSED_T_END) > 1e-9, lab
    outcomes = set()
    for key in Q.SHARED:
        for p, (c, n0, n1) in enumerate(Q.fused_reference(key, 2, False)):
            after = Q.control(2, n0, n1, c, Q.FUSED_T_END)
            outcomes.add((after[Q.C_ACCEPT], after[Q.C_DONE]))
    assert outcomes == {(1.0, 1.0), (1.0, 0.0), (0.0, 0.0)}, outcomes


def test_controller_branches_by_hand():
    """The machine at each of its branch points, against values worked out by hand."""
    c = Q.control(0, 0.9e-5, 5.0, Q.ctl_block(0), 1.0)
    assert c[Q.C_H0] == 1e-6
    c = Q.control(0, 5.0, 0.9e-5, Q.ctl_block(0), 1.0)
    assert c[Q.C_H0] == 1e-6
    c = Q.control(0, 8.0, 2.0, Q.ctl_block(0), 1.0)
    assert c[Q.C_H0] == 0.01 * 8.0 / 2.0
    c = Q.control(1, 0.5e-15 * 4e-3, 0.0, Q.ctl_block(0, h0=4e-3, d1=1e-16), 1.0)
    assert c[Q.C_H] == max(1e-6, 4e-6)
    c = Q.control(1, 2e-3, 0.0, Q.ctl_block(0, h0=1e-6, d1=3.0), 1.0)
    assert c[Q.C_H] == 100.0 * 1e-6 and c[Q.C_D2] == 2e-3 / 1e-6             # the 100 h0 cap
    for ratio, accept, fac in ((0.0, 1, 10.0), (1e-8, 1, 10.0), (0.5, 1, 0.9 / 0.5 ** 0.2), (0.9, 1, 1.0), (1.0, 1, 0.9),
                               (2.0, 0, 0.9 / 2.0 ** 0.2), (1e6, 0, 0.2), (math.inf, 0, 0.2)):
        c = Q.control(2, ratio, 0.0, Q.ctl_block(0, h=0.125, t=0.25, nacc=2), 1.0)
        assert c[Q.C_ACCEPT] == accept and c[Q.C_H] == 0.125 * fac and c[Q.C_DONE] == 0.0, ratio
        assert c[Q.C_T] == (0.375 if accept else 0.25) and c[Q.C_NACC] == (3 if accept else 2)
    c = Q.control(2, math.nan, 0.0, Q.ctl_block(0, h=0.125, t=0.25, nacc=2), 1.0)
    assert c[Q.C_ACCEPT] == 0.0 and c[Q.C_DONE] == 0.0 and c[Q.C_T] == 0.25 and c[Q.C_NACC] == 2
    c = Q.control(2, 0.5, 0.0, Q.ctl_block(0, h=0.25, t=0.75, nacc=2), 1.0)   # t + h == t_end
    assert c[Q.C_DONE] == 1.0 and c[Q.C_X] == 1.0 and c[Q.C_T] == 0.75 and c[Q.C_H] == 0.25 and c[Q.C_NACC] == 2
    c = Q.control(2, 0.5, 0.0, Q.ctl_block(0, h=0.5, t=0.75, nacc=2), 1.0)
    assert c[Q.C_DONE] == 1.0 and c[Q.C_X] == 0.5
    c = Q.control(2, 0.5, 0.0, Q.ctl_block(0, h=0.125, t=0.25, nacc=2), 1.0, n_slots=3)   # no slot left
    assert c[Q.C_OVF] == 1.0 and c[Q.C_DONE] == 1.0 and c[Q.C_NACC] == 2 and c[Q.C_T] == 0.375
