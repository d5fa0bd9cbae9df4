"""The references and bars of ``task_kernels_common`` are themselves checked, on the CPU: against the oracle's
restatements in float64 (1e-12), the float32 evaluation of every reference within half its bar on every shared case
(the condition that fixes ``K``), deliberately wrong float32 variants leaving the bar on the shared inputs (the cases
can see these bugs), and the conditions the cases are meant to meet."""
import math
import types

import numpy as np
import pytest
import torch

import task_kernels_common as T
from oracle import nlbac_oracle as O

F32, F64 = torch.float32, torch.float64


def rel(a, b):
    a, b = (v.double() if torch.is_tensor(v) else torch.tensor(v, dtype=F64) for v in (a, b))
    return float((a - b).abs().max() / b.abs().max())


def d64(t):
    return {k: v.double() for k, v in t.items()}


# ---------------------------------------------------------------------------
# every (operation, case) the float32 reference is held to half the bar on
# ---------------------------------------------------------------------------
def uni_obs(t):
    return T.unicycle_obs(t, *T.UNI_GOAL)


def uni_obs_bwd(t):
    return T.unicycle_obs_bwd(t, *T.UNI_GOAL)


def pv_obs(t):
    return T.pvtol_obs(t, t["op_prev"].shape[0], T.FOLLOW, *T.PV_GOAL)


def pv_obs_bwd(t):
    return T.pvtol_obs_bwd(t, T.FOLLOW, *T.PV_GOAL)


def obs_cases(B):
    """[(op, label, fn, inputs)] of the observation kernels on n = 2B rows (pvtol) / B rows (unicycle)."""
    g = T.gen(300 + B)
    out = []
    x = T.goal_states(B, 3, T.UNI_GOAL)
    out.append(("unicycle_obs", "B%d" % B, uni_obs, dict(x=x)))
    for acc in (0, 1):
        t = dict(x=x, dobs=T.randn(g, B, 7))
        if acc:
            t["dx0"] = T.randn(g, B, 3)
        out.append(("unicycle_obs_bwd", "B%d acc%d" % (B, acc), uni_obs_bwd, t))
    n = 2 * B
    x6 = T.goal_states(n, 6, T.PV_GOAL)
    for rows in (B, n):
        out.append(("pvtol_obs", "n%d op_rows%d" % (n, rows), pv_obs, dict(x=x6, op_prev=x6[:rows, 0] + T.randn(g, rows))))
    for acc in (0, 1):
        t = dict(x=x6, dobs=T.randn(g, n, 11))
        if acc:
            t["dx0"] = T.randn(g, n, 6)
        out.append(("pvtol_obs_bwd", "n%d acc%d" % (n, acc), pv_obs_bwd, t))
    return out


def geometry_cases(B):
    g = T.gen(400 + B)
    x = T.goal_states(2 * B, 3, T.UNI_GOAL)
    out = [("state_ps", "B%d" % B, lambda t: dict(ps=T.unicycle_state(t, T.L_P)["ps"]), dict(obs=T.state_obs(B, 9))),
           ("lookahead", "n%d" % (2 * B), lambda t: T.lookahead(t, T.L_P), dict(x=x))]
    t = dict(x=x, dps=T.randn(g, 2 * B, 2))
    out.append(("lookahead_bwd", "n%d" % (2 * B), lambda q: T.lookahead_bwd(q, T.L_P), t))
    out.append(("lookahead_bwd", "n%d dps2" % (2 * B), lambda q: T.lookahead_bwd(q, T.L_P),
                dict(t, dps2=T.randn(g, 2 * B, 2))))
    return out


TASKS = (("unicycle", 2), ("cars", 2), ("pvtol", 1), ("pvtol", 2), ("barrier", 2))


def terms_cases(B):
    out = []
    for task, NP in TASKS:
        t, p = T.terms_case(task, B, NP)
        out.append((task + "_terms", "B%d NP%d" % (B, NP), lambda q, task=task, p=p: T.TERMS[task](q, p), t))
        matr, bmatr = T.host_masks(task, B, NP)
        tb, p, mask, bmask, batch = T.bwd_inputs(task, B, NP, matr, bmatr)
        bwd = lambda q, a=(task, p, mask, bmask, batch): T.terms_bwd(a[0], q, *a[1:])
        out.append((task + "_terms_bwd", "B%d NP%d" % (B, NP), bwd, tb))
    return out


def auglag_fn(a, rho, brho):
    return lambda t: T.auglag_step(t, a, rho, brho)[0]


def all_cases():
    for B in T.ROWS:
        for c in obs_cases(B) + geometry_cases(B) + terms_cases(B):
            yield c
    for label, t, a, rho, brho in T.auglag_cases():
        yield ("auglag", label, auglag_fn(a, rho, brho), t)


def worst_float32_ratios():
    """operation -> the worst float32-reference / bar ratio over its cases (at the K of the table)."""
    worst = {}
    for op, label, fn, inputs in all_cases():
        ref, bar = T.reference_and_bar(op, fn, inputs)
        out = T.run(fn, inputs, F32)
        for k in ref:
            r = T.bar_ratio(out[k].numpy(), ref[k], bar[k])
            if r > worst.get(op, (0.0, ""))[0] or op not in worst:
                worst[op] = (r, "%s %s" % (label, k))
    return worst


def test_float32_reference_stays_within_half_the_bar():
    worst = worst_float32_ratios()
    assert set(worst) == set(T.K)
    for op, (r, where) in sorted(worst.items()):
        print("float32 reference / bar  %-20s K %3d  %.3f  (%s)" % (op, T.K[op], r, where))
    for op, (r, where) in worst.items():
        assert r <= 0.5, "%s: the float32 reference reaches %.3f of the bar at %s" % (op, r, where)


# ---------------------------------------------------------------------------
# the references against the oracle's restatements, float64
# ---------------------------------------------------------------------------
def test_state_maps_match_the_oracle():
    obs = T.state_obs(257, 9)
    st = T.unicycle_state(dict(obs=obs), T.L_P, 2)["state"]
    assert torch.equal(st[:257], O.OracleUnicycleAgent.get_state(obs)) and torch.equal(st[257:], st[:257])
    st7, st6 = O.OraclePvtolAgent.get_state(obs)
    mine = T.pvtol_state(dict(obs=obs))
    assert torch.equal(mine["st6"], st6) and torch.equal(mine["op"], st7[:, 6])
    # the special points: pi, -pi (sin = -0.0), 0, +-pi/2
    np.testing.assert_array_equal(st[:5, 2].numpy(), T.SPECIAL_ANGLES)
    cars = torch.randn(257, 12, generator=T.gen(3))
    assert torch.equal(torch.from_numpy(T.cars_state(cars.numpy())), O.OracleCarsAgent.get_state(cars[:, :10]))
    state = O.OracleCarsAgent.get_state(cars[:, :10])
    assert torch.equal(torch.from_numpy(T.cars_obs(state.numpy())), O.OracleCarsAgent.get_obs(state))


def test_lookahead_and_unicycle_terms_match_the_oracle():
    x = T.goal_states(600, 3, T.UNI_GOAL).double()
    assert rel(T.lookahead(dict(x=x), O.L_P)["ps"], O.OracleUnicycleAgent._lookahead(None, x)) <= 1e-12
    t, p = T.terms_case("unicycle", 600)
    t = d64(t)
    hr = 0.6
    ns = types.SimpleNamespace(env=types.SimpleNamespace(hazards_radius=hr, dt=p["dt"]), hazards=t["hazards"],
                               gamma_b=p["gamma_b"])
    out = T.unicycle_terms(t, dict(p, r2=(1.05 * hr) ** 2))
    assert rel(out["matr"][:, :7], O.OracleUnicycleAgent._cbf_terms(ns, t["ps"], t["ps_next"][:600])) <= 1e-12
    assert rel(out["bmatr"], O.OracleUnicycleAgent._cbf_terms(ns, t["ps"], t["ps_next"][600:])) <= 1e-12


def test_cars_terms_match_the_oracle():
    t, p = T.terms_case("cars", 600)
    t = d64(t)
    zero_policy = {"%s.%s" % (n, w): torch.zeros(s, dtype=F64) for n, s1, s2 in
                   (("linear1", (1, 10), (1,)), ("linear2", (1, 1), (1,)), ("mean_linear", (1, 1), (1,)),
                    ("log_std_linear", (1, 1), (1,))) for w, s in (("weight", s1), ("bias", s2))}
    for k, key in ((0, "matr"), (1, "bmatr")):
        steps = iter((t["x1"][k * 600:(k + 1) * 600], t["x2"][k * 600:(k + 1) * 600]))
        ns = types.SimpleNamespace(gamma_b=p["gamma_b"], get_state=lambda obs: t["state"], get_obs=O.OracleCarsAgent.get_obs,
                                   _rollout=lambda *a: (next(steps), {}), scale=torch.ones(1, dtype=F64),
                                   bias=torch.zeros(1, dtype=F64))
        batch = dict(obs=None, t=torch.zeros(600), next_t=torch.zeros(600))
        cbf = O.OracleCarsAgent._terms(ns, batch, None, zero_policy, torch.zeros(600, 1, dtype=F64), False)[0]
        assert rel(T.cars_terms(t, dict(p, radius=4.5))[key][:, :2], cbf) <= 1e-12


def _pvtol_stand_in(t, p, hr, od):
    env = types.SimpleNamespace(hazards_radius=hr, operator_dist=od, y_max=p["y_max"], y_min=p["y_min"],
                                safety_operator_follow=p["follow"])
    ns = types.SimpleNamespace(env=env, hazards=t["hazards"], gamma_b=p["gamma_b"], GOAL=T.PV_GOAL)
    ns._rd3 = lambda *h: O.OraclePvtolAgent._rd3(ns, *h)
    return ns


def test_pvtol_terms_and_obs_match_the_oracle():
    B = 600
    t, p = T.terms_case("pvtol", B, 2)
    t = d64(t)
    hr, od = 0.5, 1.0
    ns = _pvtol_stand_in(t, p, hr, od)
    out = T.pvtol_terms(t, dict(p, r2=(1.2 * hr) ** 2, d_op=0.9 * od))
    for k, key in ((0, "matr"), (1, "bmatr")):
        states = [torch.cat((t["st6"], t["op0"][:, None]), 1)]
        for n in ("x1", "x2", "x3"):
            states.append(O.OraclePvtolAgent._step7(ns, states[-1], t[n][k * B:(k + 1) * B]))
        assert rel(out[key][:, :9], O.OraclePvtolAgent._cbf_terms(ns, states)) <= 1e-12
    # get_obs of the state _step7 leaves, op_prev broadcast over the two problems' rows (i % op_rows)
    x6 = T.goal_states(2 * B, 6, T.PV_GOAL).double()
    for rows in (B, 2 * B):
        op_prev = x6[:rows, 0] + 0.5
        prev7 = torch.cat((x6, op_prev.repeat(2 * B // rows)[:, None]), 1)
        want = O.OraclePvtolAgent.get_obs(ns, O.OraclePvtolAgent._step7(ns, prev7, x6))
        got = T.pvtol_obs(dict(x=x6, op_prev=op_prev), rows, p["follow"], *T.PV_GOAL)
        assert rel(got["obs"], want) <= 1e-12 and rel(got["op"], want[:, 7]) <= 1e-12


def test_unicycle_obs_matches_the_oracle():
    x = T.goal_states(600, 3, T.UNI_GOAL).double()
    ns = types.SimpleNamespace(GOAL=T.UNI_GOAL)
    assert rel(T.unicycle_obs(dict(x=x), *T.UNI_GOAL)["obs"], O.OracleUnicycleBarrierAgent.get_obs(ns, x)) <= 1e-12


@pytest.mark.parametrize("ratio_mode,own_rho,flags", [(1, False, (1, 1)), (2, True, (1, 1)), (2, False, (0, 0)),
                                                      (1, True, (1, 0))])
def test_auglag_step_matches_the_oracle(ratio_mode, own_rho, flags):
    g = T.gen(50 + ratio_mode)
    n_cbf, rho, brho = 7, 1.3, 57.0
    t = d64(dict(partials=T.rand(g, 3, 15) * 40 + 1, lam=T.rand(g, 8) * 5, blam=T.rand(g, 7) * 5))
    t["lam"][0], t["lam"][1], t["blam"][0], t["blam"][1] = -300.0, 399.9375, -250.0, 399.9375
    a = dict(T.auglag_args(n_cbf, 1, 300.0, ratio_mode, 2 if own_rho else 1, *flags), lam_lo=0.01)
    out, rho1, brho1 = T.auglag_step(t, a, rho, brho)
    ns = types.SimpleNamespace(OWN_BACKUP_RHO=own_rho, args=types.SimpleNamespace(Lagrangian_multiplier_update_interval=2),
                               _backup_lam_mul=lambda: 1, cost_limit=0.0, RATIO_MIN=0.002 if ratio_mode == 2 else None,
                               LAM_HI=400.0, augmented_term=rho, backup_augmented_term=brho, augmented_ratio=1.0005)
    s = t["partials"].sum(0) / a["batch_size"]
    for backup, (r_k, l_k, c_k, p_k), due in ((False, ("req", "lam", "coef", "pl2"), flags[0]),
                                              (True, ("breq", "blam", "bcoef", "bpl2"), flags[1])):
        required = (s[8:] if backup else s[:8]).clone().requires_grad_(True)
        lambdas = [float(v) for v in (t["blam"] if backup else t["lam"])]
        res = O.OracleAgentBase._auglag(ns, required, lambdas, 0 if due else 1, not backup, backup)
        coef, = torch.autograd.grad(res["loss"], required)
        assert rel(out[r_k], required.detach()) <= 1e-12 and rel(out[l_k], lambdas) <= 1e-12
        assert rel(out[c_k], coef) <= 1e-12 and rel(out[p_k], res["loss"].detach()) <= 1e-12
        if not backup:
            assert rel(out["ratio"], res["ratio"]) <= 1e-12
    assert (rho1, brho1) == (ns.augmented_term, ns.backup_augmented_term)
    if flags[0]:
        assert float(out["lam"][0]) == 0.01 and float(out["lam"][1]) == 400.0     # both sides of the clamp


# ---------------------------------------------------------------------------
# mutation checks: float32 transliterations of the hand-written backward kernels, right and deliberately wrong
# ---------------------------------------------------------------------------
f = np.float32


def model_obs_bwd(x, d, goal, cols, dx0=None, accumulate=0, follow=None, bug=""):
    """unicycle_obs_bwd (cols = (4, 5, 6)) / pvtol_obs_bwd (cols = (8, 9, 10), follow given), float32 numpy."""
    x, d = x.numpy(), d.numpy()
    px, py, th = x[:, 0], x[:, 1], x[:, 2]
    c, s = np.cos(th), np.sin(th)
    rx, ry = f(goal[0]) - px, f(goal[1]) - py
    dist = np.sqrt(rx * rx + ry * ry)
    v0, v1 = c * rx + s * ry, -s * rx + c * ry
    nv = np.sqrt(v0 * v0 + v1 * v1)
    div = nv + f(0.001)
    d4, d5, d6 = (d[:, k] for k in cols)
    gpx, gpy, gth = d[:, 0].copy(), d[:, 1].copy(), -s * d[:, 2] + c * d[:, 3]
    if follow is not None:
        gpx = gpx + f(follow) * d[:, 7]
    dv0, dv1 = d4 / div, d5 / div
    dnv = -(d4 * v0 + d5 * v1) / (div * div)
    pos = nv > 0
    safe = np.where(pos, nv, f(1))
    dv0 = dv0 + np.where(pos, dnv * v0 / safe, f(0))
    dv1 = dv1 + np.where(pos, dnv * v1 / safe, f(0))
    drx, dry = dv0 * c - dv1 * s, dv0 * s + dv1 * c
    if bug != "no cross term":
        gth = gth + (dv0 * v1 - dv1 * v0)
    posd = dist > 0
    safed = np.where(posd, dist, f(1))
    dd = -d6 * np.exp(-dist)
    drx = drx + np.where(posd, dd * rx / safed, f(0))
    dry = dry + np.where(posd, dd * ry / safed, f(0))
    g = np.zeros_like(x)
    g[:, 0], g[:, 1], g[:, 2] = gpx - drx, gpy - dry, gth
    if follow is not None:
        g[:, 3], g[:, 4], g[:, 5] = d[:, 4], d[:, 5], d[:, 6]
    if accumulate and bug != "ignores accumulate":
        g = dx0.numpy() + g
    return dict(dx=g)


def model_unicycle_bwd(t, p, matr, bmatr, batch, bug=""):
    ps_next, hz, coef, bcoef = (t[k].numpy() for k in ("ps_next", "hazards", "coef", "bcoef"))
    matr, bmatr = matr.numpy(), bmatr.numpy()
    B = matr.shape[0]
    div = f(B) if bug == "/B" else f(batch)
    n, b = ps_next[:B], (ps_next[:B] if bug == "backup rows at i" else ps_next[B:])
    d, e = np.zeros((B, 2), f), np.zeros((B, 2), f)
    for h in range(7):
        g = -((coef[h] / div) / f(p["dt"]))
        d += np.where(matr[:, h:h + 1] > 0, g * (n - hz[h]), f(0))
        g = -((bcoef[h] / div) / f(p["dt"]))
        e += np.where(bmatr[:, h:h + 1] > 0, g * (b - hz[h]), f(0))
    return dict(dps_next=np.concatenate([d, e]), dV_next=np.where(matr[:, 7] > 0, (coef[7] / div) / f(p["dt"]), f(0)))


def model_cars_bwd(t, p, matr, bmatr, batch, bug=""):
    B, gb = matr.shape[0], f(p["gamma_b"])
    dx1, dx2 = np.zeros((2 * B, 10), f), np.zeros((2 * B, 10), f)
    c1 = (f(1) - gb) if bug == "single d/dh1" else -(f(-1) + gb) + (f(1) - gb)
    for k, (m, coef) in enumerate(((matr.numpy(), t["coef"].numpy()), (bmatr.numpy(), t["bcoef"].numpy()))):
        g23 = np.where(m[:, 0] > 0, coef[0] / f(batch), f(0))
        g34 = np.where(m[:, 1] > 0, coef[1] / f(batch), f(0))
        a, b = dx1[k * B:(k + 1) * B], dx2[k * B:(k + 1) * B]
        a[:, 4], a[:, 6], a[:, 8] = g23 * c1, -(g23 * c1) + g34 * c1, -(g34 * c1)
        b[:, 4], b[:, 6], b[:, 8] = -g23, g23 - g34, g34
    return dict(dx1=dx1, dx2=dx2, dV1=np.where(matr.numpy()[:, 2] > 0, t["coef"].numpy()[2] / f(batch), f(0)))


def model_pvtol_bwd(t, p, matr, bmatr, batch, bug=""):
    B, NP, fo = matr.shape[0], p["NP"], f(p["follow"])
    a = f(p["gamma_b"]) - f(1)
    ck = [f(-3) * a if bug == "ck" else f(-3) * a * a, f(-3) * a, f(-1)]
    hz = t["hazards"].numpy()
    outs = [np.zeros((NP * B, 6), f) for _ in range(3)]
    for k in range(NP):
        m = (matr if k == 0 else bmatr).numpy()
        coef = (t["coef"] if k == 0 else t["bcoef"]).numpy()
        xs = [t[n].numpy()[k * B:(k + 1) * B] for n in ("x1", "x2", "x3")]
        gx, gy, gop = ([np.zeros(B, f) for _ in range(3)] for _ in range(3))
        on = lambda c: np.where(m[:, c] > 0, coef[c] / f(batch), f(0))
        for h in range(5):
            for j in range(3):
                gx[j] += on(h) * ck[j] * (xs[j][:, 0] - hz[h, 0])
                gy[j] += on(h) * ck[j] * (xs[j][:, 1] - hz[h, 1])
        for j in range(3):
            gx[j] += on(5) * ck[j]
            gop[j] -= on(5) * ck[j]
            gx[j] -= on(6) * ck[j]
            gop[j] += on(6) * ck[j]
            gy[j] -= on(7) * ck[j]
            gy[j] += on(8) * ck[j]
        carry = f(0) if bug == "no carry" else f(1) - fo
        gx[2] += fo * gop[2]
        gop[1] += carry * gop[2]
        gx[1] += fo * gop[1]
        gop[0] += carry * gop[1]
        gx[0] += fo * gop[0]
        for j in range(3):
            outs[j][k * B:(k + 1) * B, 0], outs[j][k * B:(k + 1) * B, 1] = gx[j], gy[j]
    return dict(dx1=outs[0], dx2=outs[1], dx3=outs[2],
                dV1=np.where(matr.numpy()[:, 9] > 0, t["coef"].numpy()[9] / f(batch), f(0)))


def worst(out, ref, bar):
    return max(T.bar_ratio(np.asarray(out[k]), ref[k], bar[k]) for k in ref if k in out)


def _bwd_setup(task, B=600, NP=2):
    matr, bmatr = T.host_masks(task, B, NP)
    t, p, mask, bmask, batch = T.bwd_inputs(task, B, NP, matr, bmatr)
    ref, bar = T.reference_and_bar(task + "_terms_bwd", lambda q: T.terms_bwd(task, q, p, mask, bmask, batch), t)
    return t, p, matr, bmatr, batch, ref, bar


@pytest.mark.parametrize("task,model,bugs", [
    ("unicycle", model_unicycle_bwd, ("/B", "backup rows at i")),
    ("cars", model_cars_bwd, ("single d/dh1",)),
    ("pvtol", model_pvtol_bwd, ("ck", "no carry"))])
def test_wrong_constraint_backwards_leave_the_bar(task, model, bugs):
    t, p, matr, bmatr, batch, ref, bar = _bwd_setup(task)
    assert worst(model(t, p, matr, bmatr, batch), ref, bar) <= 1.0        # the kernel's own arithmetic stays inside
    for bug in bugs:
        assert worst(model(t, p, matr, bmatr, batch, bug), ref, bar) > 1.0, bug
    if task == "cars":      # the columns the kernel leaves zero are zero in the reference too
        others = [c for c in range(10) if c not in (4, 6, 8)]
        assert float(ref["dx1"][:, others].abs().max()) == 0.0 and float(ref["dx2"][:, others].abs().max()) == 0.0
    if task == "pvtol":
        assert max(float(ref[k][:, 2:].abs().max()) for k in ("dx1", "dx2", "dx3")) == 0.0


@pytest.mark.parametrize("task", ["unicycle", "pvtol"])
def test_wrong_observation_kernels_leave_the_bar(task):
    B = 600
    g = T.gen(8)
    goal, w, cols, follow = ((T.UNI_GOAL, 3, (4, 5, 6), None) if task == "unicycle"
                             else (T.PV_GOAL, 6, (8, 9, 10), T.FOLLOW))
    x = T.goal_states(B, w, goal)
    fwd, bwd = (uni_obs, uni_obs_bwd) if task == "unicycle" else (pv_obs, pv_obs_bwd)
    # forward without the 0.001
    inputs = dict(x=x) if task == "unicycle" else dict(x=x, op_prev=T.randn(g, B))
    ref, bar = T.reference_and_bar(task + "_obs", fwd, inputs)
    wrong = (T.unicycle_obs(inputs, *goal, offset=0.0) if task == "unicycle"
             else T.pvtol_obs(inputs, B, follow, *goal, offset=0.0))
    assert worst({k: v.numpy() for k, v in T.run(fwd, inputs, F32).items()}, ref, bar) <= 0.5
    assert T.bar_ratio(wrong["obs"][1:].numpy(), ref["obs"][1:], bar["obs"][1:]) > 1.0       # (row 0: 0 / 0 on the goal)
    # backward
    t = dict(x=x, dobs=T.randn(g, B, 7 if task == "unicycle" else 11), dx0=T.randn(g, B, w))
    ref, bar = T.reference_and_bar(task + "_obs_bwd", bwd, t)
    args = (t["x"], t["dobs"], goal, cols, t["dx0"], 1, follow)
    assert worst(model_obs_bwd(*args), ref, bar) <= 1.0
    for bug in ("no cross term", "ignores accumulate"):
        assert worst(model_obs_bwd(*args, bug=bug), ref, bar) > 1.0, bug
    # the row on the goal: finite, and the compass / distance norms hand nothing on (only d obs / d x through v / 0.001)
    row = ref["dx"][0]
    assert bool(torch.isfinite(ref["dx"]).all())
    d, th = t["dobs"][0].double(), x[0, 2].double()
    c, s = torch.cos(th), torch.sin(th)
    dv0, dv1 = d[cols[0]] / 0.001, d[cols[1]] / 0.001
    want0 = d[0] + (follow * d[7] if follow is not None else 0.0) - (dv0 * c - dv1 * s) + t["dx0"][0, 0].double()
    want2 = -s * d[2] + c * d[3] + t["dx0"][0, 2].double()
    assert abs(float(row[0] - want0)) <= 1e-9 * abs(float(want0)) and abs(float(row[2] - want2)) <= 1e-12


def test_wrong_unicycle_terms_leave_the_bar():
    t, p = T.terms_case("unicycle", 600)
    ref, bar = T.reference_and_bar("unicycle_terms", lambda q: T.unicycle_terms(q, p), t)

    def wrong(q):         # gamma_b * hn for gamma_b * hs
        hs = T._hz(q["ps"], q["hazards"], p["r2"])
        hn = T._hz(q["ps_next"][:600], q["hazards"], p["r2"])
        return -((hn - hs) / p["dt"]) - p["gamma_b"] * hn
    assert T.bar_ratio(wrong(t).numpy(), ref["matr"][:, :7], bar["matr"][:, :7]) > 1.0


def test_wrong_auglag_steps_leave_the_bar():
    cases = {label: (t, a, rho, brho) for label, t, a, rho, brho in T.auglag_cases()}
    t, a, rho, brho = cases["blk3 cbf7 clf1 ratio1 backup1 flags11 rho1"]
    ref, bar = T.reference_and_bar("auglag", auglag_fn(a, rho, brho), t)
    t32 = {k: v.float() for k, v in t.items()}
    good, rho1, _ = T.auglag_step(t32, a, rho, brho)
    assert worst({k: v.detach().numpy() for k, v in good.items()}, ref, bar) <= 0.5
    assert rho1 == min(min(rho * 1.0005, 200) * 1.0005, 200)
    # backup_mode 1 with the shared rho multiplied once per step: the backup steps from the un-multiplied rho
    once, _, r_once = T.auglag_step(t32, dict(a, backup_mode=2), rho, rho)
    assert r_once == min(rho * 1.0005, 200)
    assert worst({k: v.detach().numpy() for k, v in once.items()}, ref, bar) > 1.0
    # no clamp on the low side
    no_lo, _, _ = T.auglag_step(t32, dict(a, lam_lo=-math.inf), rho, brho)
    assert worst({k: v.detach().numpy() for k, v in no_lo.items()}, ref, bar) > 1.0


# ---------------------------------------------------------------------------
# what the cases are meant to contain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [b for b in T.ROWS if b > 1])
def test_constraint_cases_have_active_and_inactive_rows_and_signed_zeros(B):
    for task, NP in TASKS:
        matr, bmatr = T.host_masks(task, B, NP)
        t, p = T.terms_case(task, B, NP)
        out = T.run(lambda q: T.TERMS[task](q, p), t, F64)
        for key, m in (("matr", matr), ("bmatr", bmatr)):
            if m is None:
                continue
            share = (out[key] > 0).double().mean(0)
            assert float(share.min()) > 0.0 and float(share.max()) < 1.0, (task, NP, key, share)
            z = m.numpy()[m.numpy() == 0]
            assert (~np.signbit(z)).any() and np.signbit(z).any(), (task, key)
        nc = T.widths(task, NP)[0]
        assert float(torch.relu(out["matr"][:, nc - 1]).sum()) > 0.0       # the CLF required sum: the ratio is finite


def test_auglag_cases_cover_what_they_claim():
    seen = set()
    for label, t, a, rho, brho in T.auglag_cases():
        out, rho1, brho1 = T.auglag_step(d64(t), a, rho, brho)
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), label
        seen.add((a["ratio_mode"], a["backup_mode"], a["do_lambda_update"], a["do_backup_lambda_update"]))
        if a["do_lambda_update"] and not label.startswith("zero"):
            assert float(out["lam"][0]) == a["lam_lo"] and (len(out["lam"]) < 2 or float(out["lam"][1]) == a["lam_hi"])
        if a["do_backup_lambda_update"] and a["backup_mode"] and not label.startswith("zero"):
            assert float(out["blam"][0]) == a["lam_lo"] and (len(out["blam"]) < 2 or float(out["blam"][1]) == a["lam_hi"])
        if rho == 199.95:
            assert rho1 == 200.0
        if label == "zero cbf sums ratio2":
            assert float(out["ratio"]) == 0.002
        if label == "zero cbf sums ratio1":
            assert float(out["ratio"]) == 0.0
    assert {(r, b) for r, b, _, _ in seen} == {(r, b) for r in (0, 1, 2) for b in (0, 1, 2)}
    assert {(x, y) for _, _, x, y in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}
