"""The per-row task kernels of ``csrc/agent_kernels.hip`` and the augmented-Lagrangian step of ``csrc/auglag_device.h``,
each launched on its own through the C ABI and held to the float64 references and bars of ``task_kernels_common``
(``K`` fixed on the CPU, see there) and to ``vec_close(..., 1e-4)``; the maps that are one IEEE operation are held to
exact equality.  Row counts 1, 255, 257, 600: the ragged last block and 1, 2, 3 partial blocks.  Every output has a
guard row (partials: a guard block) and NaN prefill; leading dimensions are wider than the logical width.  Each check
prints its device / bar ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import task_kernels_common as T
from common import vec_close

pytestmark = pytest.mark.gpu
NAN = float("nan")


def lib():
    from nlbac_amd import _lib
    return _lib


def stream():
    from nlbac_amd.arena import stream_ptr
    return stream_ptr()


def dev(t):
    return t.contiguous().cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def padded(t, ld, g):
    """(n, w) -> device (n, ld) with the extra columns random."""
    buf = torch.randn(t.shape[0], ld, generator=g)
    buf[:, :t.shape[1]] = t
    return dev(buf)


def out_buf(rows, ld=1, fill=None):
    """(rows + 1, ld) on the device: NaN (or ``fill`` (rows, ld)) with a guard row of sentinels."""
    buf = torch.full((rows + 1, ld), NAN)
    if fill is not None:
        buf[:rows] = fill.reshape(rows, ld)
    buf[rows] = T.SENTINEL
    return dev(buf)


def read(buf, rows, width, what):
    """The (rows, width) the kernel owns, after checking that it wrote nothing else: guard row and padding untouched."""
    h = buf.cpu()
    assert bool((h[rows] == T.SENTINEL).all()), "%s: the guard row was written" % what
    assert bool(torch.isnan(h[:rows, width:]).all()), "%s: the padding columns were written" % what
    return h[:rows, :width]


def compare(op, fn, inputs, got, what):
    """Every tensor of ``got`` against the float64 reference of ``fn`` at ``inputs``: bar, then vec_close 1e-4."""
    ref, bar = T.reference_and_bar(op, fn, inputs)
    ratios = {k: T.bar_ratio(x.numpy(), ref[k], bar[k]) for k, x in got.items()}
    for k, r in ratios.items():
        print("device / bar  %-20s %-10s %-28s %.3f" % (op, k, what, r))
    for k, r in ratios.items():
        assert r <= 1.0, "%s %s (%s): %.3f of the bar (K = %d)" % (op, k, what, r, T.K[op])
        vec_close(got[k].numpy(), ref[k].numpy(), 1e-4, "%s %s (%s)" % (op, k, what))
    return ref, bar


def ulps_of(a, want):
    return np.abs(a.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ---------------------------------------------------------------------------
# observation -> state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", T.ROWS)
@pytest.mark.parametrize("n_copies,with_ps", [(1, True), (2, True), (2, False)])
def test_unicycle_and_pvtol_state(B, n_copies, with_ps):
    obs = T.state_obs(B, 9)
    d_obs = dev(obs)
    state, ps = out_buf(n_copies * B, 3), out_buf(B, 2) if with_ps else None
    lib().call("nlbac_unicycle_state", d_obs.data_ptr(), 9, B, T.L_P, state.data_ptr(), n_copies, ptr(ps), stream())
    st6, op = out_buf(B, 6), out_buf(B) if with_ps else None
    lib().call("nlbac_pvtol_state", d_obs.data_ptr(), 9, B, st6.data_ptr(), ptr(op), stream())
    torch.cuda.synchronize()
    want = T.angle_of(obs)
    k = min(B, len(T.SPECIAL_ANGLES))
    st = read(state, n_copies * B, 3, "state")
    for c in range(n_copies):
        rows = st[c * B:(c + 1) * B]
        assert torch.equal(rows[:, :2], obs[:, :2])
        th = rows[:, 2].numpy()
        print("angle, worst ulps off arctan2: %.2f" % ulps_of(th, want).max())
        assert ulps_of(th, want).max() <= 1.0
        np.testing.assert_array_equal(th[:k], T.SPECIAL_ANGLES[:k])
    s6 = read(st6, B, 6, "st6")
    assert torch.equal(s6[:, [0, 1, 3, 4, 5]], obs[:, [0, 1, 4, 5, 6]])
    assert ulps_of(s6[:, 2].numpy(), want).max() <= 1.0
    np.testing.assert_array_equal(s6[:k, 2].numpy(), T.SPECIAL_ANGLES[:k])
    if with_ps:
        assert torch.equal(read(op, B, 1, "op")[:, 0], obs[:, 7])
        compare("state_ps", lambda t: dict(ps=T.unicycle_state(t, T.L_P)["ps"]), dict(obs=obs),
                dict(ps=read(ps, B, 2, "ps")), "B%d" % B)


@pytest.mark.parametrize("B", T.ROWS)
def test_cars_maps_are_exact(B):
    g = T.gen(30 + B)
    obs = torch.randn(B, 12, generator=g)
    state, back, d_obs = out_buf(B, 10), out_buf(B, 10), dev(obs)
    lib().call("nlbac_cars_state", d_obs.data_ptr(), 12, B, state.data_ptr(), stream())
    lib().call("nlbac_cars_obs", state.data_ptr(), B, back.data_ptr(), stream())
    mb = torch.randn(B, 14, generator=g)
    pi2, c2_before = torch.randn(2 * B, generator=g), torch.randn(2 * B, 2, generator=g)
    st, y0_2, c1, c2 = out_buf(B, 10), out_buf(2 * B, 10), out_buf(2 * B, 2), out_buf(2 * B, 2, c2_before)
    d_mb, d_pi2 = dev(mb), dev(pi2)
    lib().call("nlbac_cars_rollout_inputs", d_mb.data_ptr(), 14, 12, 13, d_pi2.data_ptr(), B, st.data_ptr(),
               y0_2.data_ptr(), c1.data_ptr(), c2.data_ptr(), stream())
    torch.cuda.synchronize()
    s = read(state, B, 10, "cars state").numpy()
    np.testing.assert_array_equal(s, T.cars_state(obs.numpy()))
    np.testing.assert_array_equal(read(back, B, 10, "cars obs").numpy(), T.cars_obs(s))
    want = T.cars_rollout_inputs(mb.numpy(), 12, 13, pi2.numpy(), c2_before.numpy())
    for name, buf, rows, w, ref in (("state", st, B, 10, want[0]), ("y0_2", y0_2, 2 * B, 10, want[1]),
                                    ("c1", c1, 2 * B, 2, want[2]), ("c2", c2, 2 * B, 2, want[3])):
        np.testing.assert_array_equal(read(buf, rows, w, name).numpy(), ref, name)


# ---------------------------------------------------------------------------
# look-ahead point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", T.ROWS)
def test_lookahead_forward_and_backward(B):
    n, g = 2 * B, T.gen(40 + B)
    x = T.goal_states(n, 3, T.UNI_GOAL)
    d_x, ps = dev(x), out_buf(n, 2)
    lib().call("nlbac_unicycle_lookahead", d_x.data_ptr(), n, T.L_P, ps.data_ptr(), stream())
    dps, dps2 = torch.randn(n, 2, generator=g), torch.randn(n, 2, generator=g)
    dx = [out_buf(n, 3), out_buf(n, 3)]
    d_dps, d_dps2 = dev(dps), dev(dps2)
    lib().call("nlbac_unicycle_lookahead_bwd", d_x.data_ptr(), d_dps.data_ptr(), None, n, T.L_P, dx[0].data_ptr(), stream())
    lib().call("nlbac_unicycle_lookahead_bwd", d_x.data_ptr(), d_dps.data_ptr(), d_dps2.data_ptr(), n, T.L_P,
               dx[1].data_ptr(), stream())
    torch.cuda.synchronize()
    compare("lookahead", lambda t: T.lookahead(t, T.L_P), dict(x=x), dict(ps=read(ps, n, 2, "ps")), "n%d" % n)
    compare("lookahead_bwd", lambda t: T.lookahead_bwd(t, T.L_P), dict(x=x, dps=dps), dict(dx=read(dx[0], n, 3, "dx")),
            "n%d" % n)
    compare("lookahead_bwd", lambda t: T.lookahead_bwd(t, T.L_P), dict(x=x, dps=dps, dps2=dps2),
            dict(dx=read(dx[1], n, 3, "dx")), "n%d dps2" % n)


# ---------------------------------------------------------------------------
# get_obs and its backward
# ---------------------------------------------------------------------------
def goal_row_close(got, ref, what):
    """The row on the goal against the reference's convention, at a handful of float32 roundings of the row's scale."""
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), what
    err = float((got - ref).abs().max() / ref.abs().max())
    print("row on the goal, %s: %.2e of its scale" % (what, err))
    assert err <= 16 * 2.0 ** -24, what


@pytest.mark.parametrize("B", T.ROWS)
def test_unicycle_obs_forward_and_backward(B):
    g = T.gen(50 + B)
    x = T.goal_states(B, 3, T.UNI_GOAL)
    fwd = lambda t: T.unicycle_obs(t, *T.UNI_GOAL)
    d_x, obs = dev(x), out_buf(B, 9)
    lib().call("nlbac_unicycle_obs_fwd", d_x.data_ptr(), B, *T.UNI_GOAL, obs.data_ptr(), 9, stream())
    dobs, dx0 = torch.randn(B, 7, generator=g), torch.randn(B, 3, generator=g)
    d_dobs = padded(dobs, 9, g)
    dx = [out_buf(B, 3), out_buf(B, 3, dx0)]
    for acc in (0, 1):
        lib().call("nlbac_unicycle_obs_bwd", d_x.data_ptr(), d_dobs.data_ptr(), 9, B, *T.UNI_GOAL, dx[acc].data_ptr(), acc,
                   stream())
    torch.cuda.synchronize()
    o = read(obs, B, 7, "obs")
    compare("unicycle_obs", fwd, dict(x=x), dict(obs=o), "B%d" % B)
    assert o[0, 4:].tolist() == [0.0, 0.0, 1.0]          # on the goal: compass 0 / 0.001, exp(-0)
    for acc in (0, 1):
        t = dict(x=x, dobs=dobs, **(dict(dx0=dx0) if acc else {}))
        got = read(dx[acc], B, 3, "dx")
        ref, _ = compare("unicycle_obs_bwd", lambda q: T.unicycle_obs_bwd(q, *T.UNI_GOAL), t, dict(dx=got),
                         "B%d acc%d" % (B, acc))
        goal_row_close(got[0], ref["dx"][0], "unicycle_obs_bwd acc%d" % acc)


@pytest.mark.parametrize("B", T.ROWS)
def test_pvtol_obs_forward_and_backward(B):
    n, g = 2 * B, T.gen(60 + B)
    x = T.goal_states(n, 6, T.PV_GOAL)
    d_x = dev(x)
    for rows, with_op in ((B, True), (n, False), (n, True)):
        op_prev = x[:rows, 0] + torch.randn(rows, generator=g)
        obs, op_out, d_op = out_buf(n, 13), out_buf(n) if with_op else None, dev(op_prev)
        lib().call("nlbac_pvtol_obs_fwd", d_x.data_ptr(), d_op.data_ptr(), rows, T.FOLLOW, *T.PV_GOAL, n,
                   obs.data_ptr(), 13, ptr(op_out), stream())
        torch.cuda.synchronize()
        got = dict(obs=read(obs, n, 11, "obs"))
        if with_op:
            got["op"] = read(op_out, n, 1, "op")[:, 0]
            assert torch.equal(got["op"], got["obs"][:, 7])
        compare("pvtol_obs", lambda t: T.pvtol_obs(t, rows, T.FOLLOW, *T.PV_GOAL), dict(x=x, op_prev=op_prev), got,
                "n%d op_rows%d" % (n, rows))
        assert got["obs"][0, 8:].tolist() == [0.0, 0.0, 1.0]
        assert torch.equal(got["obs"][:, [0, 1, 4, 5, 6]], x[:, [0, 1, 3, 4, 5]])
    dobs, dx0 = torch.randn(n, 11, generator=g), torch.randn(n, 6, generator=g)
    d_dobs = padded(dobs, 13, g)
    dx = [out_buf(n, 6), out_buf(n, 6, dx0)]
    for acc in (0, 1):
        lib().call("nlbac_pvtol_obs_bwd", d_x.data_ptr(), d_dobs.data_ptr(), 13, T.FOLLOW, *T.PV_GOAL, n, dx[acc].data_ptr(),
                   acc, stream())
    torch.cuda.synchronize()
    for acc in (0, 1):
        t = dict(x=x, dobs=dobs, **(dict(dx0=dx0) if acc else {}))
        got = read(dx[acc], n, 6, "dx")
        ref, _ = compare("pvtol_obs_bwd", lambda q: T.pvtol_obs_bwd(q, T.FOLLOW, *T.PV_GOAL), t, dict(dx=got),
                         "n%d acc%d" % (n, acc))
        goal_row_close(got[0], ref["dx"][0], "pvtol_obs_bwd acc%d" % acc)


# ---------------------------------------------------------------------------
# CBF / CLF terms, forward (unfused) and backward
# ---------------------------------------------------------------------------
def launch_fwd(task, d, p, B, NP, matr, bmatr, partials, fused=None, ticket=None, sc=None):
    """One ``*_constraints_fwd`` launch on the device tensors ``d``."""
    tail = (None if fused is None else C.byref(fused), ptr(ticket), ptr(sc), stream())
    if task == "unicycle":
        lib().call("nlbac_unicycle_constraints_fwd", d["ps"].data_ptr(), d["ps_next"].data_ptr(), d["V"].data_ptr(),
                   d["V_next"].data_ptr(), d["hazards"].data_ptr(), 7, p["r_coll"], p["dt"], p["gamma_b"], p["gamma_l"], B,
                   matr.data_ptr(), bmatr.data_ptr(), partials.data_ptr(), *tail)
    elif task == "cars":
        lib().call("nlbac_cars_constraints_fwd", d["state"].data_ptr(), d["x1"].data_ptr(), d["x2"].data_ptr(),
                   d["V"].data_ptr(), d["V1"].data_ptr(), p["gamma_b"], p["gamma_l"], p["radius"], B, matr.data_ptr(),
                   bmatr.data_ptr(), partials.data_ptr(), *tail)
    elif task == "pvtol":
        lib().call("nlbac_pvtol_constraints_fwd", d["st6"].data_ptr(), d["op0"].data_ptr(), d["x1"].data_ptr(),
                   d["x2"].data_ptr(), d["x3"].data_ptr(), d["V"].data_ptr(), d["V1"].data_ptr(), d["hazards"].data_ptr(), 5,
                   p["r_coll"], p["d_op"], p["y_max"], p["y_min"], p["follow"], p["gamma_b"], p["gamma_l"], B, NP,
                   matr.data_ptr(), ptr(bmatr), partials.data_ptr(), *tail)
    else:
        lib().call("nlbac_barrier_constraints_fwd", d["Bv"].data_ptr(), d["Bn"].data_ptr(), d["V"].data_ptr(),
                   d["Vn"].data_ptr(), p["dt"], p["gamma_b"], p["gamma_l"], B, matr.data_ptr(), partials.data_ptr(), *tail)


def launch_bwd(task, d, p, B, NP, matr, bmatr, batch, sc, outs):
    o = [b.data_ptr() for b in outs]
    if task == "unicycle":
        lib().call("nlbac_unicycle_constraints_bwd", d["ps_next"].data_ptr(), matr.data_ptr(), bmatr.data_ptr(),
                   d["hazards"].data_ptr(), 7, p["dt"], batch, B, sc.data_ptr(), *o, stream())
    elif task == "cars":
        lib().call("nlbac_cars_constraints_bwd", matr.data_ptr(), bmatr.data_ptr(), p["gamma_b"], batch, B, sc.data_ptr(),
                   *o, stream())
    elif task == "pvtol":
        lib().call("nlbac_pvtol_constraints_bwd", matr.data_ptr(), ptr(bmatr), d["x1"].data_ptr(), d["x2"].data_ptr(),
                   d["x3"].data_ptr(), d["hazards"].data_ptr(), 5, p["follow"], p["gamma_b"], batch, B, NP, sc.data_ptr(),
                   *o, stream())
    else:
        lib().call("nlbac_barrier_constraints_bwd", matr.data_ptr(), p["dt"], batch, B, sc.data_ptr(), *o, stream())


TASKS = (("unicycle", 2), ("cars", 2), ("pvtol", 1), ("pvtol", 2), ("barrier", 2))


@pytest.mark.parametrize("B", T.ROWS)
@pytest.mark.parametrize("task,NP", TASKS)
def test_constraint_terms_forward_and_backward(task, NP, B):
    t, p = T.terms_case(task, B, NP)
    d = {k: dev(v) for k, v in t.items()}
    nc, nb = T.widths(task, NP)
    n_blk, what = (B + 255) // 256, "B%d NP%d" % (B, NP)
    matr, bmatr, partials = out_buf(B, nc), out_buf(B, nb) if nb else None, out_buf(n_blk, nc + nb)
    launch_fwd(task, d, p, B, NP, matr, bmatr, partials)
    torch.cuda.synchronize()
    got = dict(matr=read(matr, B, nc, "matr"))
    if nb:
        got["bmatr"] = read(bmatr, B, nb, "bmatr")
    ref, bar = compare(task + "_terms", lambda q: T.TERMS[task](q, p), t, got, what)
    # the per-block partials [blk][ncol]: float64 sums of the block's relu'd terms, the bar summed over the block
    part = read(partials, n_blk, nc + nb, "partials")
    r = T.bar_ratio(part.numpy(), T.block_sums(ref["relu"]), T.block_sums(bar["relu"]))
    print("device / bar  %-20s %-10s %-28s %.3f" % (task + "_terms", "partials", what, r))
    assert r <= 1.0
    vec_close(part.numpy(), T.block_sums(ref["relu"]).numpy(), 1e-4, "partials")
    # backward on the device's own term matrices, a few entries set to 0.0 / -0.0; batch_size = 3 B
    m_h = T.with_signed_zeros(got["matr"])
    b_h = T.with_signed_zeros(got["bmatr"]) if nb else None
    tb, p, mask, bmask, batch = T.bwd_inputs(task, B, NP, m_h, b_h)
    sc = dev(T.coefs(task, NP))
    shapes = {"unicycle": ((2 * B, 2), (B, 1)), "cars": ((2 * B, 10), (2 * B, 10), (B, 1)),
              "pvtol": ((NP * B, 6), (NP * B, 6), (NP * B, 6), (B, 1)), "barrier": ((B, 1), (B, 1))}[task]
    outs = [out_buf(*s) for s in shapes]
    d_m, d_b = dev(m_h), dev(b_h) if nb else None
    launch_bwd(task, d, p, B, NP, d_m, d_b, batch, sc, outs)
    torch.cuda.synchronize()
    assert torch.equal(sc.cpu(), T.coefs(task, NP))
    names = ["d" + n for n in T.LEAVES[task]]
    got = {n: read(o, s[0], s[1], n) for n, o, s in zip(names, outs, shapes)}
    got = {n: (v[:, 0] if s[1] == 1 else v) for (n, v), s in zip(got.items(), shapes)}
    ref, _ = compare(task + "_terms_bwd", lambda q: T.terms_bwd(task, q, p, mask, bmask, batch), tb, got, what)
    if task == "cars":          # the columns the kernel must leave zero
        others = [c for c in range(10) if c not in (4, 6, 8)]
        assert float(got["dx1"][:, others].abs().max()) == 0.0 and float(got["dx2"][:, others].abs().max()) == 0.0
    if task == "pvtol":
        assert max(float(got[k][:, 2:].abs().max()) for k in ("dx1", "dx2", "dx3")) == 0.0


def fused_args(a):
    A = lib().AuglagArgs()
    for k, v in a.items():
        setattr(A, k, v)
    return A


@pytest.mark.parametrize("task", ["unicycle", "cars", "pvtol", "barrier"])
def test_fused_tail_leaves_the_scalars_of_the_two_launches(task):
    """constraints_fwd with the ticket and the step's arguments == the unfused launch + nlbac_auglag on its partials."""
    B, NP = 600, 2
    n_cbf, n_clf, ratio_mode, backup_mode, lam_hi = T.AUGLAG_TASKS[task]
    a = T.auglag_args(n_cbf, n_clf, float(B), ratio_mode, backup_mode, lam_hi=lam_hi)
    t, p = T.terms_case(task, B, NP)
    d = {k: dev(v) for k, v in t.items()}
    nc, nb = T.widths(task, NP)
    g = T.gen(70)
    sc0 = torch.from_numpy(T.sc_block(dict(lam=torch.rand(nc, generator=g) * 5, blam=torch.rand(n_cbf, generator=g) * 5),
                                      1.7, 3.1))
    res = []
    for fused in (False, True):
        matr, bmatr, partials = out_buf(B, nc), out_buf(B, nb) if nb else None, out_buf(3, nc + nb)
        sc, ticket = dev(sc0), torch.zeros(4, dtype=torch.int32, device="cuda")
        if fused:
            launch_fwd(task, d, p, B, NP, matr, bmatr, partials, fused_args(a), ticket, sc)
        else:
            launch_fwd(task, d, p, B, NP, matr, bmatr, partials)
            lib().call("nlbac_auglag", partials.data_ptr(), 3, n_cbf, n_clf, a["batch_size"], 1, 1, ratio_mode, backup_mode,
                       a["lam_lo"], a["lam_hi"], sc.data_ptr(), stream())
        torch.cuda.synchronize()
        assert int(ticket.abs().sum().item()) == 0
        res.append((sc.cpu(), read(matr, B, nc, "matr"), read(partials, 3, nc + nb, "partials")))
    for x, y in zip(*res):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(res[0][0], sc0)
    keep = T.sc_untouched(sc0.numpy(), a)
    np.testing.assert_array_equal(res[1][0].numpy().view(np.int32)[keep], sc0.numpy().view(np.int32)[keep])


# ---------------------------------------------------------------------------
# the augmented-Lagrangian step alone
# ---------------------------------------------------------------------------
def launch_auglag(partials, n_blk, a, sc):
    lib().call("nlbac_auglag", partials.data_ptr(), n_blk, a["n_cbf"], a["n_clf"], a["batch_size"], a["do_lambda_update"],
               a["do_backup_lambda_update"], a["ratio_mode"], a["backup_mode"], a["lam_lo"], a["lam_hi"], sc.data_ptr(),
               stream())


def check_auglag(label, t, a, rho, brho, before, after):
    want, rho1, brho1 = T.auglag_step({k: v.double() for k, v in t.items()}, a, rho, brho)
    got, rho_d, brho_d = T.sc_outputs(after, a)
    compare("auglag", lambda q: T.auglag_step(q, a, rho, brho)[0], t,
            {k: torch.as_tensor(np.asarray(v, dtype=np.float32).reshape(want[k].shape)) for k, v in got.items()}, label)
    # rho is a double, stepped as Python steps it: min(rho * 1.0005, 200), twice where the backup shares it
    assert (rho_d, brho_d) == (rho1, brho1), (label, rho_d, rho1, brho_d, brho1)
    keep = T.sc_untouched(before, a)
    np.testing.assert_array_equal(after.view(np.int32)[keep], before.view(np.int32)[keep], label)


def test_auglag_step_modes_clamps_and_write_back_window():
    cases = T.auglag_cases()
    before = np.stack([T.sc_block(t, rho, brho, seed=100 + i) for i, (_, t, a, rho, brho) in enumerate(cases)])
    sc = dev(torch.from_numpy(before))
    parts = [dev(t["partials"]) for _, t, _, _, _ in cases]
    for i, (label, t, a, rho, brho) in enumerate(cases):
        launch_auglag(parts[i], t["partials"].shape[0], a, sc[i])
    torch.cuda.synchronize()
    after = sc.cpu().numpy()
    for i, (label, t, a, rho, brho) in enumerate(cases):
        check_auglag(label, t, a, rho, brho, before[i], after[i])


@pytest.mark.parametrize("n_cbf,backup_mode", [(7, 1), (9, 2)])
def test_auglag_sums_700_blocks_in_staging_rounds_exactly(n_cbf, backup_mode):
    """700 blocks at 15 / 19 columns: more than the 307 / 242 blocks one staging round holds.  The partials are small
    integers times 2^-6, so every float32 sum is exact and the required sums are one division away."""
    nc, ncol, n_blk = n_cbf + 1, 2 * n_cbf + 1, 700
    P = T.exact_partials(n_blk, ncol)
    g = T.gen(80)
    t = dict(partials=P, lam=torch.rand(nc, generator=g) * 5, blam=torch.rand(n_cbf, generator=g) * 5)
    a = T.auglag_args(n_cbf, 1, 179200.0, 2, backup_mode)
    before = T.sc_block(t, 1.0, 1.0)
    sc = dev(torch.from_numpy(before))
    d_P = dev(P)
    launch_auglag(d_P, n_blk, a, sc)
    torch.cuda.synchronize()
    after = sc.cpu().numpy()
    sums = P.double().sum(0).numpy()
    assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)
    want = sums.astype(np.float32) / np.float32(a["batch_size"])
    np.testing.assert_array_equal(after[T.SC_REQ:T.SC_REQ + nc], want[:nc])
    np.testing.assert_array_equal(after[T.SC_BREQ:T.SC_BREQ + n_cbf], want[nc:])
    check_auglag("700 blocks, %d columns" % ncol, t, a, 1.0, 1.0, before, after)
