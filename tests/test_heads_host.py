"""The references, bars and shared cases of ``heads_common`` are themselves checked, on the CPU: the float32 evaluation
of every reference within half its bar on every shared case (the condition that fixes ``K``), the caps on ill-conditioned
elements, the references against independent float64 formulations (``torch.distributions.Normal``, plain autograd
through ``torch.clamp`` / ``torch.min``, ``torch.nn.functional.mse_loss``), float32 transliterations of the kernels'
arithmetic — right ones inside the bar, deliberately wrong ones outside it on the shared inputs —, and the regimes the
cases are meant to hold."""
import numpy as np
import pytest
import torch

import heads_common as H

F32, F64 = torch.float32, torch.float64


def rel(a, b):
    a, b = (v.double() if torch.is_tensor(v) else torch.tensor(v, dtype=F64) for v in (a, b))
    return float((a - b).abs().max() / b.abs().max())


def d64(t):
    return {k: v.double() for k, v in t.items()}


@pytest.fixture(scope="module")
def measured():
    """[(op, label, name, float32 / bar, ill-conditioned share)] over every shared case and output."""
    rows = []
    for op, label, fn, inputs, noise in H.shared_cases():
        ref, bar = H.reference_and_bar_noisy(op, fn, inputs, noise)
        out = H.run(fn, inputs, F32)
        for k in ref:
            rows.append((op, label, k, H.bar_ratio(out[k].numpy(), ref[k], bar[k]), H.ill_share(ref[k], bar[k])))
    return rows


# ---------------------------------------------------------------------------
# K, and the caps that keep a wide bar from hiding a failure
# ---------------------------------------------------------------------------
def test_float32_reference_stays_within_half_the_bar_and_k_is_the_smallest(measured):
    worst = {}
    for op, label, k, r, _ in measured:
        if op not in worst or r > worst[op][0]:
            worst[op] = (r, "%s %s" % (label, k))
    assert set(worst) == set(H.K)
    for op, (r, where) in sorted(worst.items()):
        print("float32 reference / bar  %-16s K %3d  %.3f  (%s)" % (op, H.K[op], r, where))
    for op, (r, where) in worst.items():
        assert r <= 0.5, "%s: the float32 reference reaches %.3f of the bar at %s" % (op, r, where)
        # the bar is linear in K: half of K would not do
        assert H.K[op] == 1 or 2 * r > 0.5, "%s: K = %d is not the smallest (%.3f)" % (op, H.K[op], r)


NO_ILL = {("gauss_fwd", "action"), ("td_targets", "dq"), ("td_targets", "next_q"), ("td_targets", "next_l"),
          ("td_value", "dpred"), ("td_value", "next_out"), ("actor_q", "dq1"), ("actor_q", "dq2"), ("mse", "dpred")}
QUARTER = {("gauss_fwd", "logp"), ("gauss_bwd", "dheads")}


def test_ill_conditioned_elements_are_capped(measured):
    seen = set()
    for op, label, k, _, share in measured:
        seen.add((op, k))
        if (op, k) in QUARTER:
            assert share <= 0.25, "%s %s (%s): %.3f of the elements are ill-conditioned" % (op, k, label, share)
        else:       # every other tensor, those of NO_ILL among them
            assert share == 0.0, "%s %s (%s): %.3f of the elements are ill-conditioned" % (op, k, label, share)
    assert NO_ILL <= seen and QUARTER <= seen
    worst = max(s for op, _, k, _, s in measured if (op, k) in QUARTER)
    print("largest ill-conditioned share of logp / dheads: %.3f" % worst)
    assert worst > 0.0          # the saturated rows are there


def test_action_bars_stay_at_rounding_size():
    for B in H.ROWS:
        for n_u in range(1, H.MAX_NU + 1):
            t, _ = H.gauss_case(B, n_u)
            ref, bar = H.reference_and_bar_noisy("gauss_fwd", lambda q: H.gauss_fwd(q, n_u), t, H.gauss_noise(t))
            assert float(bar["action"].max()) <= 1e-6 * float(ref["action"].abs().max()) * H.K["gauss_fwd"]


# ---------------------------------------------------------------------------
# the references against independent float64 formulations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_u", [1, 2, 3, 4])
def test_gauss_forward_matches_torch_distributions(n_u):
    t, _ = H.gauss_case(600, n_u)
    t = d64(t)
    got = H.gauss_fwd(t, n_u)
    mean, ls = t["heads"][:, :n_u], t["heads"][:, n_u:].clamp(-20, 2)
    normal = torch.distributions.Normal(mean, ls.exp())
    x = mean + t["eps"] * ls.exp()
    y = torch.tanh(x)
    logp = normal.log_prob(x) - torch.log(t["scale"] * (1 - y.pow(2)) + 1e-6)
    assert rel(got["action"], y * t["scale"] + t["bias"]) <= 1e-12
    assert rel(got["logp"], logp.sum(1)) <= 1e-12
    assert H.LOG_SQRT_2PI == pytest.approx(0.91893853320467274178, abs=1e-15)
    assert rel(H.gauss_x(t, n_u), x) <= 1e-15


def plain_gauss_bwd(t, n_u, rows_per_problem, dlogp_mul, sample_eps=1e-6):
    """The gradient by plain autograd through torch.clamp / torch.tanh / Normal.log_prob, float64."""
    heads = t["heads"].detach().clone().requires_grad_(True)
    mean, ls = heads[:, :n_u], heads[:, n_u:].clamp(-20, 2)
    std = ls.exp()
    x = mean + t["eps"] * std
    y = torch.tanh(x)
    action = y * t["scale"] + t["bias"]
    logp = (torch.distributions.Normal(mean, std).log_prob(x) - torch.log(t["scale"] * (1 - y.pow(2)) + sample_eps)).sum(1)
    da = sum(t["da%d" % k][:, :n_u] for k in range(3) if "da%d" % k in t) if "da0" in t else torch.zeros_like(action)
    dlp = t["alpha"][torch.arange(heads.shape[0]) // rows_per_problem] * dlogp_mul
    g, = torch.autograd.grad((da * action).sum() + (dlp * logp).sum(), heads)
    return g


@pytest.mark.parametrize("n_u,n_src,P,norm_mul", H.GAUSS_BWD_VARIANTS)
def test_gauss_backward_matches_plain_autograd_and_the_clamp_passes_its_boundaries(n_u, n_src, P, norm_mul):
    B = 600
    fn, t, _, B_norm, mul = H.gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
    _, reg = H.gauss_bwd_case(B, n_u, n_src, P)
    got = fn(d64(t))["dheads"]
    want = plain_gauss_bwd(d64(t), n_u, B, mul)
    # plain autograd adds and removes eps / std * d logp in d mean: float64 carries that where std is not tiny
    ok = torch.from_numpy(~np.isin(reg, [H.GAUSS_REGIMES.index(r) for r in ("min", "below_min", "far_below",
                                                                                "min_with_mean")]))
    assert rel(got[ok], want[ok]) <= 1e-10
    assert float((got[~ok] - want[~ok]).abs().max()) <= 1e-6 * float(want.abs().max())
    # inclusive boundaries: torch.clamp itself hands the gradient on at exactly -20 and exactly 2, not one step outside
    dls, plain_dls = got[:, n_u:], want[:, n_u:]
    for name, zero in (("min", False), ("max", False), ("below_min", True), ("above_max", True), ("far_below", True),
                       ("far_above", True)):
        rows = torch.from_numpy(reg == H.GAUSS_REGIMES.index(name))
        assert int(rows.sum()) >= H.PER_REGIME
        for d in (dls, plain_dls):
            assert bool((d[rows] == 0).all()) if zero else bool((d[rows] != 0).all()), name


@pytest.mark.parametrize("norm_mul", [1, 2])
def test_td_references_match_mse_loss_autograd(norm_mul):
    B = 600
    B_norm = norm_mul * B
    t = d64(H.td_inputs(H.td_case(B)))
    got = H.td_targets(t, H.GAMMA, B_norm, H.f32(1.0 / B_norm))
    with torch.no_grad():
        mq = torch.min(t["q1t"], t["q2t"]) - t["alpha"] * t["nlogp"]
        next_q = t["reward"] + t["mask"] * H.GAMMA * mq
        next_l = t["constraint"] + t["mask"] * H.GAMMA * t["lt"]
    assert rel(got["next_q"], next_q) <= 1e-12 and rel(got["next_l"], next_l) <= 1e-12
    for c, (pred, target) in enumerate((("q1", next_q), ("q2", next_q), ("lf", next_l))):
        p = t[pred].clone().requires_grad_(True)
        loss = torch.nn.functional.mse_loss(p, target)          # the mean over this rank's B rows
        g, = torch.autograd.grad(loss * B / B_norm, p)
        assert rel(got["dq"][:, c], g) <= 1e-12
        assert rel(got["losses"][c], loss.detach() * B * H.f32(1.0 / B_norm)) <= 1e-12
    v = d64(H.td_value_inputs(H.td_case(B)))
    got = H.td_value(v, H.GAMMA, B_norm, H.f32(1.0 / B_norm))
    y = v["signal"] + v["mask"] * H.GAMMA * v["next_target"]
    p = v["pred"].clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(p, y)
    g, = torch.autograd.grad(loss * B / B_norm, p)
    assert rel(got["dpred"], g) <= 1e-12 and rel(got["next_out"], y) <= 1e-12
    assert rel(got["loss"], loss.detach() * B * H.f32(1.0 / B_norm)) <= 1e-12


@pytest.mark.parametrize("P", [1, 2])
def test_actor_references_match_torch_min_autograd(P):
    B = 600
    fn, t, B_norm = H.actor_q_setup(B, P)
    got = fn(d64(t))
    a, b = (t[k].double().requires_grad_(True) for k in ("q1", "q2"))
    m = torch.min(a, b)
    da, db = torch.autograd.grad(-(m.sum()) / B_norm, (a, b))
    assert torch.equal(got["dq1"], da) and torch.equal(got["dq2"], db)
    g = -1.0 / B_norm
    _, kind = H.actor_case(B, P)
    k = torch.from_numpy(kind)
    assert bool((da[k == 0] == g).all()) and bool((db[k == 0] == 0).all())
    assert bool((da[k == 1] == 0).all()) and bool((db[k == 1] == g).all())
    for tie in (2, 3, 4):
        assert bool((da[k == tie] == 0.5 * g).all()) and bool((db[k == tie] == 0.5 * g).all())
    alpha = t["alpha"].double()[torch.arange(P * B) // B]
    pl1 = (alpha * t["logp"].double() - m.detach()).view(P, B).sum(1)
    sums = got["terms"].view(P, B, 2).sum(1)
    assert rel(sums[:, 0], pl1) <= 1e-12 and rel(sums[:, 1], t["logp"].double().view(P, B).sum(1)) <= 1e-12


def test_scalar_and_mse_references():
    for first, P in H.SCALARS_VARIANTS:
        t = d64(H.scalars_inputs(3, first, P))
        got = H.actor_scalars(t, 768.0, first, P, H.TARGET_ENTROPY)
        s = t["partials"][first:first + P].sum(1)
        assert rel(got["mean_logp"], s[:, 1] / 768.0) <= 1e-15 and rel(got["pl1"], s[:, 0] / 768.0) <= 1e-15
        assert rel(got["aloss"], -(t["log_alpha"] * (s[:, 1] / 768.0 + H.TARGET_ENTROPY))) <= 1e-15
        assert rel(got["g_log_alpha"], -(s[:, 1] / 768.0 + H.TARGET_ENTROPY)) <= 1e-15
    for d, _, norm_mul in H.MSE_SHAPES:
        n = 257
        t = d64(H.mse_case(n, d))
        got = H.mse(t, norm_mul * n)
        p = t["pred"].clone().requires_grad_(True)
        loss = torch.nn.functional.mse_loss(p, t["target"])
        g, = torch.autograd.grad(loss / norm_mul, p)
        assert rel(got["dpred"], g) <= 1e-12 and rel(got["e2"].sum() / (n * d), loss.detach()) <= 1e-12


# ---------------------------------------------------------------------------
# mutation checks: float32 transliterations of the kernels' arithmetic, right and deliberately wrong
# ---------------------------------------------------------------------------
def model_gauss_bwd(t, n_u, rows_per_problem, dlogp_mul, bug=""):
    """``gauss_bwd_one`` (csrc/dy_heads.h), float32 torch."""
    heads, e = t["heads"], t["eps"]
    mean, raw = heads[:, :n_u], heads[:, n_u:]
    ls = torch.clamp(raw, H.LOG_SIG_MIN, H.LOG_SIG_MAX)
    std = torch.exp(ls)
    y = torch.tanh(mean + e * std)
    da = torch.zeros_like(mean)
    for k in range(3):
        if "da%d" % k in t:
            da = da + t["da%d" % k][:, :n_u]
    dlp = (t["alpha"][torch.arange(heads.shape[0]) // rows_per_problem] * np.float32(dlogp_mul))[:, None]
    s1 = t["scale"] * (1.0 - y * y)
    sample_eps = 0.0 if bug == "no SAMPLE_EPS" else np.float32(H.SAMPLE_EPS)
    gx = da * s1 + dlp * (2.0 * y * s1 / (s1 + sample_eps))
    dstd = gx * e
    in_range = ((raw > H.LOG_SIG_MIN) & (raw < H.LOG_SIG_MAX)) if bug == "exclusive clamp" else H.inside_of(heads, n_u)
    dls = torch.where(in_range, dstd * std - dlp, torch.zeros_like(dstd))
    return dict(dheads=torch.cat((gx, dls), 1))


def worst(out, ref, bar):
    return max(H.bar_ratio(np.asarray(out[k]), ref[k], bar[k]) for k in ref if k in out)


def test_wrong_gauss_backwards_leave_the_bar():
    caught = {"no SAMPLE_EPS": 0, "exclusive clamp": 0, "B for B_norm": 0}
    for B in (257, 600):
        for n_u, n_src, P, norm_mul in H.GAUSS_BWD_VARIANTS:
            fn, t, noise, B_norm, mul = H.gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
            ref, bar = H.reference_and_bar_noisy("gauss_bwd", fn, t, noise)
            assert worst(model_gauss_bwd(t, n_u, B, mul), ref, bar) <= 1.0       # the kernel's own arithmetic stays inside
            for bug in ("no SAMPLE_EPS", "exclusive clamp"):
                caught[bug] += worst(model_gauss_bwd(t, n_u, B, mul, bug), ref, bar) > 1.0
            if norm_mul != 1:
                caught["B for B_norm"] += worst(model_gauss_bwd(t, n_u, B, H.f32(1.0 / B)), ref, bar) > 1.0
    print(caught)
    assert caught["no SAMPLE_EPS"] == 8 and caught["exclusive clamp"] == 8 and caught["B for B_norm"] == 4


def model_actor_q(t, B, B_norm, P, bug=""):
    """``actor_q_terms_kernel``'s row arithmetic, float32 torch."""
    a, b = t["q1"], t["q2"]
    g = -(np.float32(1.0) / np.float32(B if bug == "B for B_norm" else B_norm))
    half = np.float32(0.5) * g
    zero = torch.zeros_like(a)
    if bug == "tie to one side":
        dq1, dq2 = torch.where(a <= b, g, zero), torch.where(b < a, g, zero)
    else:
        dq1 = torch.where(a < b, g, torch.where(a == b, half, zero))
        dq2 = torch.where(b < a, g, torch.where(a == b, half, zero))
    alpha = t["alpha"][torch.arange(P * B) // B]
    return dict(dq1=dq1, dq2=dq2, terms=torch.stack([alpha * t["logp"] - torch.minimum(a, b), t["logp"]], 1))


def test_wrong_actor_terms_leave_the_bar():
    for B in (257, 600):
        for P in (1, 2):
            fn, t, B_norm = H.actor_q_setup(B, P)
            ref, bar = H.reference_and_bar_noisy("actor_q", fn, t)
            assert worst(model_actor_q(t, B, B_norm, P), ref, bar) <= 1.0
            assert worst(model_actor_q(t, B, B_norm, P, "tie to one side"), ref, bar) > 1.0
            if B_norm != B:
                assert worst(model_actor_q(t, B, B_norm, P, "B for B_norm"), ref, bar) > 1.0


def model_td(t, gamma, B_norm, bug=""):
    """``td_targets_kernel``'s row arithmetic, float32 torch."""
    mk = torch.ones_like(t["mask"]) if bug == "ignores the mask" else t["mask"]
    g = np.float32(gamma)
    mq = torch.minimum(t["q1t"], t["q2t"]) - t["alpha"][0] * t["nlogp"]
    yq = t["reward"] + mk * g * mq
    yl = t["constraint"] + mk * g * t["lt"]
    norm = np.float32(2.0 / B_norm)
    e = torch.stack([t["q1"] - yq, t["q2"] - yq, t["lf"] - yl], 1)
    return dict(next_q=yq, next_l=yl, dq=norm * e, e2=e * e)


def test_wrong_td_targets_leave_the_bar():
    for B in (257, 600):
        t = H.td_inputs(H.td_case(B))
        for norm_mul in (1, 2):
            B_norm = norm_mul * B
            ref, bar = H.reference_and_bar_noisy("td_targets", lambda q: H.td_targets(q, H.GAMMA, B_norm, 1.0), t)
            assert worst(model_td(t, H.GAMMA, B_norm), ref, bar) <= 1.0
            assert worst(model_td(t, H.GAMMA, B_norm, "ignores the mask"), ref, bar) > 1.0
            if norm_mul != 1:
                assert worst(model_td(t, H.GAMMA, B), ref, bar) > 1.0         # B for B_norm


# ---------------------------------------------------------------------------
# what the cases are meant to contain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 257, 510, 514, 600, 1200])
@pytest.mark.parametrize("n_u", [1, 2, 3, 4])
def test_gauss_cases_hold_every_regime(n, n_u):
    t, reg = H.gauss_case(n, n_u)
    count = lambda name: int((reg == H.GAUSS_REGIMES.index(name)).sum())
    rows = lambda name: torch.from_numpy(reg == H.GAUSS_REGIMES.index(name))
    for name in H.GAUSS_REGIMES:
        assert count(name) >= H.PER_REGIME, name
    assert reg[0] == 0
    ls = t["heads"][:, n_u:]
    for name, v in (("min", -20.0), ("max", 2.0), ("far_below", -60.0), ("far_above", 15.0), ("min_with_mean", -20.0)):
        assert bool((ls[rows(name)] == v).all())
    below, above = ls[rows("below_min")], ls[rows("above_max")]
    assert bool((below < -20.0).all()) and bool((below == np.nextafter(np.float32(-20.0), np.float32(-30.0))).all())
    assert bool((above > 2.0).all()) and bool((above == np.nextafter(np.float32(2.0), np.float32(3.0))).all())
    assert bool((t["eps"][rows("eps0")] == 0).all())
    for name in ("min", "below_min", "far_below"):
        assert bool((t["heads"][:, :n_u][rows(name)] == 0).all())
    assert bool((t["heads"][:, :n_u][rows("min_with_mean")] != 0).all())
    x = H.gauss_x(t, n_u)[rows("saturated")]
    assert float(x.abs().min()) >= 3.5 and float(x.abs().max()) <= 12.5
    assert float(x[:, 0].abs().min()) <= 4.3 and float(x[:, 0].abs().max()) >= 11.7
    y32 = torch.tanh(x.float())          # float32 tanh just below 1 and exactly +-1, both signs
    assert bool((y32.abs() == 1).any()) and bool((y32.abs() < 1).any()) and bool((y32 == 1).any()) and bool((y32 == -1).any())
    assert float(t["scale"].min()) >= 0.5 and float(t["scale"].max()) <= 2.0 and bool((t["bias"] != 0).all())


def test_backward_cases_hold_what_they_claim():
    seen_src, seen_P, seen_norm = set(), set(), set()
    for n_u, n_src, P, norm_mul in H.GAUSS_BWD_VARIANTS:
        t, _ = H.gauss_bwd_case(257, n_u, n_src, P)
        seen_src.add(n_src), seen_P.add(P), seen_norm.add(norm_mul)
        for k in range(n_src):
            assert t["da%d" % k].shape == (P * 257, n_u + 1 + k)       # each its own leading dimension, wider than n_u
        assert "da%d" % n_src not in t
        assert len(set(t["alpha"].tolist())) == P
    assert seen_src == {0, 1, 3} and seen_P == {1, 2} and seen_norm == {1, 2}


@pytest.mark.parametrize("B", [b for b in H.ROWS if b > 1])
def test_td_and_actor_cases_hold_what_they_claim(B):
    t = H.td_case(B)
    mask = t["rcm"][:, H.RCM_COLS["mask"]]
    assert set(mask.tolist()) == {0.0, 1.0} and abs(float((mask == 0).float().mean()) - 1 / 3) < 0.01
    assert int((t["q1t"] == t["q2t"]).sum()) >= H.PER_REGIME and int((t["q1t"] != t["q2t"]).sum()) >= H.PER_REGIME
    assert float(t["nlogp"].abs().max()) > 45 and float(t["nlogp"].abs().max()) <= 50
    assert H.RCM_LD > 1 and len({*H.RCM_COLS.values(), H.XSIG_COL}) == 4
    for P in (1, 2):
        q, kind = H.actor_case(B, P)
        for k in range(len(H.ACTOR_ROW_KINDS)):
            assert int((kind == k).sum()) >= H.PER_REGIME, H.ACTOR_ROW_KINDS[k]
        a, b, k = q["q1"], q["q2"], torch.from_numpy(kind)
        assert bool((a[k == 0] < b[k == 0]).all()) and bool((b[k == 1] < a[k == 1]).all())
        assert bool((a[k == 2] == b[k == 2]).all()) and bool((a[k == 2] != 0).all())
        sa, sb = np.signbit(a.numpy()), np.signbit(b.numpy())
        z3, z4 = (k == 3).numpy(), (k == 4).numpy()
        assert not sa[z3].any() and sb[z3].all() and sa[z4].all() and not sb[z4].any()
        assert bool((a[k >= 3] == 0).all()) and bool((b[k >= 3] == 0).all())
        assert len(set(q["alpha"].tolist())) == P
    assert {f for f, _ in H.SCALARS_VARIANTS} == {0, 1} and H.LOG_ALPHA_STRIDE > 1
