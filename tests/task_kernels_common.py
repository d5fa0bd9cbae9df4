"""Float64 references, shared cases and the comparator for the per-row task kernels of ``csrc/agent_kernels.hip``
(observation <-> state maps, look-ahead point, differentiable ``get_obs`` and its backward, CBF / CLF constraint terms
and their backward) and the augmented-Lagrangian step of ``csrc/auglag_device.h``.  Imports without a GPU.

References.  One plain torch function per operation, written in the formulas' own form and run in the dtype of the
tensors it is handed: float64 is the reference, float32 is the same formulas at the kernels' precision (what fixes
``K`` below).  Tensor inputs are the float32 tensors the device gets, cast up; scalar parameters are rounded to
float32 (``f32``) where the ABI takes ``float`` and ``r2`` is formed as the launchers form it (``launcher_r2``).
Every backward reference is ``torch.autograd.grad`` of the forward reference.  The constraint backward differentiates
``L = sum_c coef_c / batch_size * sum_i mask_ic term_ic`` with the mask read off the float32 ``matr`` / ``bmatr`` the
backward kernel is given and ``coef`` from the scalars block.  At the two non-differentiable points of ``get_obs``
(``|v| == 0``, ``dist == 0``) the norm contributes nothing (``_norm2``: ``torch.where`` on a safe argument), which is
the kernels' ``nv > 0`` / ``dist > 0`` convention.

Comparator.  An element may differ from the float64 reference by at most

    bar = K * ( max over 8 seeded draws of |f64(x (1 + d)) - f64(x)| + 2^-24 |f64(x)| )

with an independent d ~ U[-2^-23, 2^-23] per element of every tensor input: these maps cancel ((hn - hs) / dt,
1 / div^2 next to the goal), so the bar follows the reference's own sensitivity to an input rounding.  ``K`` comes from
the reference alone: the smallest power of two for which the float32 evaluation of the same reference stays within
HALF the bar on every shared case (``test_task_kernels_host.py`` asserts it).  It is never adjusted from a device
result.  Every tensor also meets ``common.vec_close(..., 1e-4)``.

``K`` and the worst float32-reference / bar ratio (CPU), then the worst device / bar ratio (MI355X), per operation:

    operation                K   float32 reference   device
    state_ps                 2   0.282               0.284
    lookahead                2   0.284               0.284
    lookahead_bwd            4   0.335               0.271
    unicycle_obs             8   0.271               0.271
    unicycle_obs_bwd         8   0.408               0.493
    pvtol_obs                4   0.409               0.447
    pvtol_obs_bwd            8   0.441               0.465
    unicycle_terms          32   0.413               0.413
    unicycle_terms_bwd       2   0.482               0.472
    cars_terms               1   0.484               0.484
    cars_terms_bwd           1   0.366               0.366
    pvtol_terms             64   0.345               0.345
    pvtol_terms_bwd         32   0.291               0.051
    barrier_terms            4   0.388               0.187
    barrier_terms_bwd        2   0.289               0.289
    auglag                   8   0.279               0.279
"""
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
ROWS = (1, 255, 257, 600)          # one lane per row in 256-lane blocks: ragged last block, 1 / 2 / 3 partial blocks
DRAWS = 8

# operation -> K (the table above)
K = {"state_ps": 2, "lookahead": 2, "lookahead_bwd": 4, "unicycle_obs": 8, "unicycle_obs_bwd": 8, "pvtol_obs": 4,
     "pvtol_obs_bwd": 8, "unicycle_terms": 32, "unicycle_terms_bwd": 2, "cars_terms": 1, "cars_terms_bwd": 1,
     "pvtol_terms": 64, "pvtol_terms_bwd": 32, "barrier_terms": 4, "barrier_terms_bwd": 2, "auglag": 8}

# the scalars block (csrc/scalars.h)
SC_SIZE, SC_RATIO, SC_PL2, SC_BPL2 = 128, 4, 5, 6
SC_LAMBDA, SC_BLAMBDA, SC_COEF, SC_BCOEF, SC_REQ, SC_BREQ = 16, 32, 48, 64, 80, 96
SC_RHO_F64, SC_BRHO_F64, SC_MEAN_LOGP = 112, 114, 116


def f32(v):
    """A scalar as the ABI's ``float`` argument carries it."""
    return float(np.float32(v))


def launcher_r2(r_coll):
    """``(float)((double)r * r)`` of the ``*_constraints_fwd`` launchers."""
    return float(np.float32(np.float64(np.float32(r_coll)) ** 2))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def angle_of(obs):
    """``get_state``'s heading: arctan2 in float64 on the host, cast down (numpy, exact by definition)."""
    o = obs.detach().cpu().numpy().astype(np.float64)
    return np.arctan2(o[:, 3], o[:, 2]).astype(np.float32)


def unicycle_state(t, l_p, n_copies=1):
    """obs (B, >= 4) -> state (n_copies B, 3) = [x, y, theta] and the look-ahead point ps (B, 2)."""
    obs = t["obs"]
    th = torch.from_numpy(angle_of(obs)).to(obs.dtype)
    st = torch.stack([obs[:, 0], obs[:, 1], th], 1)
    ps = torch.stack([obs[:, 0] + l_p * torch.cos(th), obs[:, 1] + l_p * torch.sin(th)], 1)
    return dict(state=st.repeat(n_copies, 1), ps=ps)


def pvtol_state(t):
    """obs (n, >= 8) -> the six dynamic states and the safety operator's position."""
    obs = t["obs"]
    th = torch.from_numpy(angle_of(obs)).to(obs.dtype)
    return dict(st6=torch.stack([obs[:, 0], obs[:, 1], th, obs[:, 4], obs[:, 5], obs[:, 6]], 1), op=obs[:, 7])


_CARS_SCALE = np.array([100.0, 30.0] * 5)


def cars_state(obs):
    """numpy float32 (n, >= 10) -> (n, 10): one double multiply and one cast per element."""
    return (obs[:, :10].astype(np.float64) * _CARS_SCALE).astype(np.float32)


def cars_obs(state):
    """numpy float32 (n, 10): one float32 division per element."""
    return state / _CARS_SCALE.astype(np.float32)


def cars_rollout_inputs(mb, t_col, nt_col, pi2, c2_before):
    """state (B, 10), its two copies (2B, 10), c1 (2B, 2) = [action, t], c2 (2B, 2) with only the time column set."""
    B = mb.shape[0]
    st = cars_state(mb)
    c1 = np.stack([pi2, np.concatenate([mb[:, t_col]] * 2)], 1)
    c2 = c2_before.copy()
    c2[:2 * B, 1] = np.concatenate([mb[:, nt_col]] * 2)
    return st, np.concatenate([st, st]), c1, c2


def lookahead(t, l_p):
    x = t["x"]
    return dict(ps=torch.stack([x[:, 0] + l_p * torch.cos(x[:, 2]), x[:, 1] + l_p * torch.sin(x[:, 2])], 1))


def lookahead_bwd(t, l_p):
    """d/dx of sum(ps * (dps [+ dps2]))."""
    x = t["x"].clone().requires_grad_(True)
    d = t["dps"] + t["dps2"] if "dps2" in t else t["dps"]
    g, = torch.autograd.grad((lookahead(dict(x=x), l_p)["ps"] * d).sum(), x)
    return dict(dx=g)


def _norm2(a, b):
    """sqrt(a^2 + b^2); at (0, 0) the value is 0 and the norm hands no gradient on."""
    q = a * a + b * b
    pos = q > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))


def _goal_features(px, py, th, gx, gy, offset):
    c, s = torch.cos(th), torch.sin(th)
    rx, ry = gx - px, gy - py
    dist = _norm2(rx, ry)
    v0, v1 = c * rx + s * ry, -s * rx + c * ry
    div = _norm2(v0, v1) + offset
    return c, s, v0 / div, v1 / div, torch.exp(-dist)


def unicycle_obs(t, gx, gy, offset=0.001):
    """x (n, 3) -> [x, y, cos, sin, compass (2), exp(-dist)]."""
    x = t["x"]
    c, s, a, b, e = _goal_features(x[:, 0], x[:, 1], x[:, 2], gx, gy, offset)
    return dict(obs=torch.stack([x[:, 0], x[:, 1], c, s, a, b, e], 1))


def pvtol_obs(t, op_rows, follow, gx, gy, offset=0.001):
    """x (n, 6), op_prev (op_rows) read at ``i % op_rows`` -> the 11 observation columns and the operator's new position."""
    x = t["x"]
    o0 = t["op_prev"][torch.arange(x.shape[0]) % op_rows]
    o1 = o0 + follow * (x[:, 0] - o0)
    c, s, a, b, e = _goal_features(x[:, 0], x[:, 1], x[:, 2], gx, gy, offset)
    return dict(obs=torch.stack([x[:, 0], x[:, 1], c, s, x[:, 3], x[:, 4], x[:, 5], o1, a, b, e], 1), op=o1)


def obs_bwd(obs_fn, t):
    """dx = [dx0 +] d/dx sum(obs(x) * dobs); ``obs_fn``: a forward reference with its scalars bound."""
    x = t["x"].clone().requires_grad_(True)
    rest = {k: v for k, v in t.items() if k not in ("x", "dobs", "dx0")}
    g, = torch.autograd.grad((obs_fn(dict(rest, x=x))["obs"] * t["dobs"]).sum(), x)
    return dict(dx=g + t["dx0"] if "dx0" in t else g)


def unicycle_obs_bwd(t, gx, gy):
    return obs_bwd(lambda q: unicycle_obs(q, gx, gy), t)


def pvtol_obs_bwd(t, follow, gx, gy):
    """(the operator's previous position does not enter d/dx: zeros serve)"""
    n = t["x"].shape[0]
    return obs_bwd(lambda q: pvtol_obs(dict(q, op_prev=torch.zeros(n, dtype=q["x"].dtype)), n, follow, gx, gy), t)


def _hz(p, hazards, r2):
    return 0.5 * (((p[:, None, :] - hazards[None]) ** 2).sum(2) - r2)


def _with_relu(matr, bmatr):
    out = dict(matr=matr, relu=torch.relu(matr))
    if bmatr is not None:
        out.update(bmatr=bmatr, relu=torch.cat((torch.relu(matr), torch.relu(bmatr)), 1))
    return out


def unicycle_terms(t, p):
    """ps (B, 2), ps_next (2B, 2): primary rows then backup rows; matr (B, 8) = [7 CBF terms, CLF], bmatr (B, 7)."""
    B = t["ps"].shape[0]
    hs = _hz(t["ps"], t["hazards"], p["r2"])
    cbf = lambda pn: -((_hz(pn, t["hazards"], p["r2"]) - hs) / p["dt"]) - p["gamma_b"] * hs
    lya = ((t["V_next"] - t["V"]) / p["dt"]) + p["gamma_l"] * t["V"]
    return _with_relu(torch.cat((cbf(t["ps_next"][:B]), lya[:, None]), 1), cbf(t["ps_next"][B:]))


def cars_terms(t, p):
    """state (B, 10), x1 / x2 (2B, 10); matr (B, 3) = [cbf23, cbf34, CLF], bmatr (B, 2)."""
    B, gb = t["state"].shape[0], p["gamma_b"]
    h = lambda x: ((x[:, 4:5] - x[:, 6:7]) - p["radius"], (x[:, 6:7] - x[:, 8:9]) - p["radius"])

    def problem(k):
        cols = []
        for h0, h1, h2 in zip(h(t["state"]), h(t["x1"][k * B:(k + 1) * B]), h(t["x2"][k * B:(k + 1) * B])):
            l1 = h1 - h0 + gb * h0
            l2 = h2 - h1 + gb * h1
            cols.append(-(l2 - l1) - gb * l1)
        return torch.cat(cols, 1)
    lya = (t["V1"] - t["V"]) + p["gamma_l"] * t["V"]
    return _with_relu(torch.cat((problem(0), lya[:, None]), 1), problem(1))


def pvtol_terms(t, p):
    """st6 (B, 6), op0 (B), x1 / x2 / x3 (NP B, 6); matr (B, 10) = [5 hazards, x - op, op - x, y_max, y_min, CLF],
    bmatr (B, 9) for NP == 2."""
    B, gb, fo = t["st6"].shape[0], p["gamma_b"], p["follow"]

    def rd3(h0, h1, h2, h3):
        t1 = h3 - h2 + gb * h2
        t2 = h2 - h1 + gb * h1
        t3 = h1 - h0 + gb * h0
        return -(t1 - t2 + gb * t2 - (t2 - t3 + gb * t3) + gb * (t2 - t3 + gb * t3))

    def problem(k):
        xs = [t["st6"]] + [t[n][k * B:(k + 1) * B] for n in ("x1", "x2", "x3")]
        ops = [t["op0"]]
        for x in xs[1:]:
            ops.append(ops[-1] + fo * (x[:, 0] - ops[-1]))
        hz = [_hz(x[:, :2], t["hazards"], p["r2"]) for x in xs]
        h1 = [(x[:, 0] - o + p["d_op"]).unsqueeze(1) for x, o in zip(xs, ops)]
        h2 = [(-x[:, 0] + o + p["d_op"]).unsqueeze(1) for x, o in zip(xs, ops)]
        h3 = [(-x[:, 1] + p["y_max"] - 10.0).unsqueeze(1) for x in xs]
        h4 = [(x[:, 1] - p["y_min"] - 10.0).unsqueeze(1) for x in xs]
        return torch.cat([rd3(*h) for h in (hz, h1, h2, h3, h4)], 1)
    lya = ((t["V1"] - t["V"]) / 1.0) + p["gamma_l"] * t["V"]
    return _with_relu(torch.cat((problem(0), lya[:, None]), 1), problem(1) if p["NP"] == 2 else None)


def barrier_terms(t, p):
    """matr (B, 2) = [-(B' - B) - gamma_b B, (V' - V) / dt + gamma_l V]."""
    bt = -(t["Bn"] - t["Bv"]) - p["gamma_b"] * t["Bv"]
    lt = ((t["Vn"] - t["V"]) / p["dt"]) + p["gamma_l"] * t["V"]
    return _with_relu(torch.stack([bt, lt], 1), None)


TERMS = {"unicycle": unicycle_terms, "cars": cars_terms, "pvtol": pvtol_terms, "barrier": barrier_terms}
LEAVES = {"unicycle": ("ps_next", "V_next"), "cars": ("x1", "x2", "V1"), "pvtol": ("x1", "x2", "x3", "V1"),
          "barrier": ("Bn", "Vn")}


def terms_bwd(task, t, p, mask, bmask, batch_size):
    """Gradients of L = sum_c coef_c / batch_size sum_i mask_ic term_ic w.r.t. the task's leaves.  ``t`` holds the
    forward's tensors plus ``coef`` (nc) and ``bcoef`` (n_cbf); the masks (0 / 1, float64) are constants."""
    leaves = [t[n].clone().requires_grad_(True) for n in LEAVES[task]]
    out = TERMS[task](dict(t, **dict(zip(LEAVES[task], leaves))), p)
    dt = leaves[0].dtype
    L = ((t["coef"] / batch_size) * (mask.to(dt) * out["matr"]).sum(0)).sum()
    if "bmatr" in out:
        L = L + ((t["bcoef"] / batch_size) * (bmask.to(dt) * out["bmatr"]).sum(0)).sum()
    return dict(zip(("d" + n for n in LEAVES[task]), torch.autograd.grad(L, leaves)))


def auglag_step(t, a, rho, brho):
    """sac_cbf_clf.py:502-528, 623-638 on the partial sums.  ``t``: partials (n_blk, ncol), lam (nc), blam (n_cbf);
    ``a``: the scalar arguments of ``nlbac_auglag``; ``rho`` / ``brho``: Python floats (doubles in the scalars block).
    Returns (dict of tensors, new rho, new brho); the coefficients are d loss / d required by autograd."""
    n_cbf, n_clf, mode = a["n_cbf"], a["n_clf"], a["backup_mode"]
    nc = n_cbf + n_clf
    s = t["partials"].sum(0) / a["batch_size"]
    req = s[:nc].detach().clone().requires_grad_(True)
    ratio = torch.ones((), dtype=s.dtype)
    if n_clf and a["ratio_mode"]:
        ratio = (torch.abs(torch.mean(req[:n_cbf])) / torch.abs(req[nc - 1])).detach()
        if a["ratio_mode"] == 2:
            ratio = torch.clamp(ratio, min=0.002)
    lam = t["lam"]
    if a["do_lambda_update"]:
        lam = torch.clamp(lam + rho * req.detach(), a["lam_lo"], a["lam_hi"])
    rho = min(rho * 1.0005, 200)
    loss = 0.0
    for c in range(n_cbf):
        loss = loss + lam[c] * req[c] + rho / 2.0 * req[c] * req[c]
    if n_clf:
        g = req[nc - 1]
        loss = loss + lam[nc - 1] * ratio * g + ratio * ratio * rho / 2.0 * g * g
    coef, = torch.autograd.grad(loss, req)
    out = dict(req=req.detach(), ratio=ratio, lam=lam, coef=coef, pl2=loss.detach())
    if mode:
        breq = s[nc:].detach().clone().requires_grad_(True)
        r = rho if mode == 1 else brho          # mode 1: the shared rho, already multiplied once this step
        blam = t["blam"]
        if a["do_backup_lambda_update"]:
            blam = torch.clamp(blam + r * breq.detach(), a["lam_lo"], a["lam_hi"])
        r = min(r * 1.0005, 200)
        bloss = 0.0
        for c in range(n_cbf):
            bloss = bloss + blam[c] * breq[c] + r / 2.0 * breq[c] * breq[c]
        bcoef, = torch.autograd.grad(bloss, breq)
        rho, brho = (r, brho) if mode == 1 else (rho, r)
        out.update(breq=breq.detach(), blam=blam, bcoef=bcoef, bpl2=bloss.detach())
    return out, rho, brho


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def run(fn, inputs, dtype):
    return {k: v.detach() for k, v in fn({k: v.to(dtype) for k, v in inputs.items()}).items()}


def reference_and_bar(op, fn, inputs, seed=0, k=None):
    """(float64 reference, bar) per output of ``fn`` (dict of tensors -> dict of tensors) at the float32 ``inputs``.
    ``k``: the bar's factor where the operation is not one of this module's (``ode_control_common``)."""
    k = K[op] if k is None else k
    base = run(fn, inputs, F64)
    dev = {k: torch.zeros_like(v) for k, v in base.items()}
    g = gen(1000 + seed)
    for _ in range(DRAWS):
        nud = {k: v.double() * (1.0 + (torch.rand(v.shape, generator=g, dtype=F64) * 2 - 1) * 2.0 ** -23)
               for k, v in inputs.items()}
        out = run(fn, nud, F64)
        dev = {k: torch.maximum(dev[k], (out[k] - base[k]).abs()) for k in base}
    return base, {name: k * (dev[name] + 2.0 ** -24 * base[name].abs()) for name in base}


def bar_ratio(x, ref, bar):
    """Worst |x - ref| / bar (0 where x == ref; inf where x is not finite or differs under a zero bar)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(ref.shape)
    err = (x - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar)
    r = torch.where(torch.isfinite(x), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def block_sums(v, block=256):
    """Per-block column sums [blk][ncol] of a (B, ncol) tensor, blocks of 256 rows."""
    return torch.stack([v[b:b + block].sum(0) for b in range(0, v.shape[0], block)])


# ---------------------------------------------------------------------------
# shared cases (float32 tensors; built once, read unchanged)
# ---------------------------------------------------------------------------
L_P = f32(0.03)
UNI_GOAL = (f32(2.5), f32(2.5))
PV_GOAL = (f32(4.5), f32(4.5))
FOLLOW = f32(0.3)
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def state_obs(B, ld, seed=1):
    """Observation rows (B, ld) whose columns 2, 3 are (cos, sin): unit-circle rows, then the special points
    (-1, 0), (-1, -0.0), (0, 0), (0, 1), (0, -1) in the first rows (as many as B holds)."""
    g = gen(seed + B)
    obs = torch.randn(B, ld, generator=g)
    th = (torch.rand(B, generator=g, dtype=F64) * 2 - 1) * math.pi
    obs[:, 2], obs[:, 3] = torch.cos(th).float(), torch.sin(th).float()
    special = torch.tensor([[-1.0, 0.0], [-1.0, -0.0], [0.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    k = min(B, len(special))
    obs[:k, 2:4] = special[:k]
    return obs


SPECIAL_ANGLES = np.array([math.pi, -math.pi, 0.0, math.pi / 2, -math.pi / 2]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def goal_states(B, width, goal, seed=2):
    """States (B, width) for the observation kernels: random rows, and in the first rows (as many as B holds) one row
    exactly on the goal, rows at distance 1e-1 .. 1e-5 from it at three bearings, and theta at 0, +-pi (float32) and
    beyond +-pi."""
    g = gen(seed + B + 7 * width)
    x = torch.randn(B, width, generator=g)
    x[:, 0] = goal[0] + (torch.rand(B, generator=g) * 2 - 1) * 3
    x[:, 1] = goal[1] + (torch.rand(B, generator=g) * 2 - 1) * 3
    x[:, 2] = (torch.rand(B, generator=g) * 2 - 1) * 3.1
    rows = [(goal[0], goal[1], 0.7)]
    for k, d in enumerate((1e-1, 1e-2, 1e-3, 1e-4, 1e-5)):
        for b in (0.3, 2.0, -2.6):
            rows.append((goal[0] + d * math.cos(b + k), goal[1] + d * math.sin(b + k), 0.4 * k - b))
    sp = torch.tensor(rows, dtype=F64).float()
    k = min(B, len(sp))
    x[:k, :3] = sp[:k]
    for j, th in enumerate((0.0, math.pi, -math.pi, 4.0, -7.5)):
        if k + j < B:
            x[k + j, 2] = th
    return x


def rand(g, *shape):
    return torch.rand(*shape, generator=g)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def terms_case(task, B, NP=2):
    """(tensors, scalar parameters) of one constraints_fwd call."""
    g = gen({"unicycle": 11, "cars": 12, "pvtol": 13, "barrier": 14}[task] * 1000 + B + NP)
    V = rand(g, B) + 0.1
    if task == "unicycle":
        ps = rand(g, B, 2) * 4 - 2
        t = dict(ps=ps, ps_next=torch.cat((ps, ps)) + 0.05 * randn(g, 2 * B, 2), V=V, V_next=V + 0.02 * randn(g, B),
                 hazards=rand(g, 7, 2) * 4 - 2)
        r = f32(1.05 * 0.6)
        p = dict(r_coll=r, r2=launcher_r2(r), dt=f32(0.02), gamma_b=f32(2.0), gamma_l=f32(1.0))
    elif task == "cars":
        st = randn(g, B, 10) * 3
        st[:, 8] = 20 + randn(g, B)
        st[:, 6] = st[:, 8] + 2 + 6 * rand(g, B)
        st[:, 4] = st[:, 6] + 2 + 6 * rand(g, B)
        x1 = torch.cat((st, st)) + randn(g, 2 * B, 10)
        t = dict(state=st, x1=x1, x2=x1 + randn(g, 2 * B, 10), V=V, V1=V + 0.3 * randn(g, B))
        p = dict(gamma_b=f32(0.5), gamma_l=f32(0.15), radius=f32(4.5))
    elif task == "pvtol":
        st = randn(g, B, 6)
        st[:, :2] = rand(g, B, 2) * 6
        x1 = torch.cat([st] * NP) + 0.5 * randn(g, NP * B, 6)
        x2 = x1 + 0.5 * randn(g, NP * B, 6)
        t = dict(st6=st, op0=st[:, 0] + 0.8 * randn(g, B), x1=x1, x2=x2, x3=x2 + 0.5 * randn(g, NP * B, 6), V=V,
                 V1=V + 0.3 * randn(g, B), hazards=rand(g, 5, 2) * 6)
        r = f32(1.2 * 0.5)
        p = dict(r_coll=r, r2=launcher_r2(r), d_op=f32(0.9), y_max=f32(15.0), y_min=f32(-9.0), follow=FOLLOW,
                 gamma_b=f32(0.8), gamma_l=f32(0.1), NP=NP)
    else:
        Bv = randn(g, B)
        t = dict(Bv=Bv, Bn=Bv + 0.5 * randn(g, B), V=V, Vn=V + 0.02 * randn(g, B))
        p = dict(dt=f32(0.02), gamma_b=f32(0.8), gamma_l=f32(1.0))
    return t, p


def widths(task, NP=2):
    """(columns of matr, columns of bmatr or 0)."""
    return {"unicycle": (8, 7), "cars": (3, 2), "pvtol": (10, 9 if NP == 2 else 0), "barrier": (2, 0)}[task]


def with_signed_zeros(m):
    """A copy of a term matrix with a few entries overwritten by 0.0 and -0.0 (inactive: gradient 0)."""
    m = m.clone()
    flat = m.view(-1)
    n = flat.numel()
    for j, v in ((0, 0.0), (n // 2, -0.0), (n - 1, 0.0), (n // 3, -0.0)):
        flat[j] = v
    return m


@functools.lru_cache(maxsize=None)
def coefs(task, NP=2, seed=5):
    """Distinct positive SC_COEF / SC_BCOEF entries and a scalars block (float32, 128) that holds them among sentinels."""
    nc, nb = widths(task, NP)
    g = gen(seed + nc)
    sc = randn(g, SC_SIZE) * 100
    sc[SC_COEF:SC_COEF + 16] = rand(g, 16) + 0.25 + torch.arange(16) * 0.125
    sc[SC_BCOEF:SC_BCOEF + 16] = rand(g, 16) + 0.3 + torch.arange(16) * 0.0625
    return sc


def bwd_inputs(task, B, NP, matr, bmatr):
    """What the backward reference needs for the float32 term matrices the backward kernel is given:
    (tensors incl. coef / bcoef, parameters, mask, bmask, batch_size = 3 B)."""
    t, p = terms_case(task, B, NP)
    nc, nb = widths(task, NP)
    sc = coefs(task, NP)
    t = dict(t, coef=sc[SC_COEF:SC_COEF + nc].clone())
    if nb:
        t["bcoef"] = sc[SC_BCOEF:SC_BCOEF + nb].clone()
    mask = (matr > 0).double()
    bmask = (bmatr > 0).double() if nb else None
    return t, p, mask, bmask, float(3 * B)


def host_masks(task, B, NP=2):
    """The float32 reference's own term matrices with the signed zeros put in (the host tests' stand-in for the device
    forward's)."""
    t, p = terms_case(task, B, NP)
    out = run(lambda q: TERMS[task](q, p), t, F32)
    return with_signed_zeros(out["matr"]), (with_signed_zeros(out["bmatr"]) if "bmatr" in out else None)


AUGLAG_TASKS = {     # task -> (n_cbf, n_clf, ratio_mode, backup_mode, lam_hi) as sac_cbf_clf/tasks.py sets them
    "unicycle": (7, 1, 1, 1, 400.0), "cars": (2, 1, 2, 1, 300.0), "pvtol": (9, 1, 2, 2, 400.0),
    "barrier": (1, 1, 0, 0, 400.0)}


def auglag_args(n_cbf, n_clf, batch_size, ratio_mode, backup_mode, do_lam=1, do_blam=1, lam_lo=0.01, lam_hi=400.0):
    return dict(n_cbf=n_cbf, n_clf=n_clf, batch_size=f32(batch_size), do_lambda_update=do_lam,
                do_backup_lambda_update=do_blam, ratio_mode=ratio_mode, backup_mode=backup_mode, lam_lo=f32(lam_lo),
                lam_hi=f32(lam_hi))


@functools.lru_cache(maxsize=None)
def auglag_cases():
    """[(label, tensors, args, rho, brho)]: n_blk 1 and 3 with random partials; every ratio_mode / backup_mode; both
    update flags on and off; multipliers that end below lam_lo, inside and above lam_hi; rho 1.0 and 199.95 (the cap
    binds); one case whose CBF sums are all zero (mode 2's 0.002 floor binds, mode 1's ratio is 0)."""
    cases = []
    g = gen(77)
    for n_blk in (1, 3):
        for (n_cbf, n_clf, backup_mode) in ((7, 1, 1), (9, 1, 2), (1, 1, 0), (2, 1, 1), (3, 0, 2)):
            nc = n_cbf + n_clf
            ncol = nc + (n_cbf if backup_mode else 0)
            for ratio_mode in (0, 1, 2):
                for flags, rho in (((1, 1), 1.0), ((0, 1), 199.95), ((1, 0), 199.95), ((0, 0), 1.0)):
                    P = rand(g, n_blk, ncol) * 40 + 1
                    lam = rand(g, nc) * 5
                    blam = rand(g, n_cbf) * 5
                    # lam + rho * req: entry 0 ends under lam_lo, entry 1 over lam_hi (req >= 0.01, rho >= 1)
                    lam[0], blam[0] = -300.0, -250.0
                    if nc > 1:
                        lam[1] = 399.999
                    if n_cbf > 1:
                        blam[1] = 399.999
                    a = auglag_args(n_cbf, n_clf, 100.0 * n_blk, ratio_mode, backup_mode, flags[0], flags[1])
                    cases.append(("blk%d cbf%d clf%d ratio%d backup%d flags%d%d rho%g" % (
                        n_blk, n_cbf, n_clf, ratio_mode, backup_mode, flags[0], flags[1], rho),
                        dict(partials=P, lam=lam, blam=blam), a, rho, 150.0 if rho == 1.0 else 199.99))
    for ratio_mode in (1, 2):          # CBF sums all zero
        P = rand(g, 3, 15) * 40
        P[:, :7] = 0.0
        a = auglag_args(7, 1, 300.0, ratio_mode, 1)
        cases.append(("zero cbf sums ratio%d" % ratio_mode, dict(partials=P, lam=rand(g, 8) * 5, blam=rand(g, 7) * 5),
                      a, 1.0, 1.0))
    return cases


def sc_block(tensors, rho, brho, seed=9):
    """A scalars block (numpy float32, 128) of sentinels with the multipliers and the two doubles put in."""
    sc = (torch.randn(SC_SIZE, generator=gen(seed)) * 100).numpy().copy()
    sc[SC_LAMBDA:SC_LAMBDA + len(tensors["lam"])] = tensors["lam"].numpy()
    sc[SC_BLAMBDA:SC_BLAMBDA + len(tensors["blam"])] = tensors["blam"].numpy()
    sc[SC_RHO_F64:SC_RHO_F64 + 4].view(np.float64)[:] = (rho, brho)
    return sc


def sc_outputs(sc, a):
    """The step's outputs read out of a scalars block (numpy float32, 128) -> (dict like ``auglag_step``'s, rho, brho)."""
    n_cbf, nc = a["n_cbf"], a["n_cbf"] + a["n_clf"]
    out = dict(req=sc[SC_REQ:SC_REQ + nc], ratio=sc[SC_RATIO], lam=sc[SC_LAMBDA:SC_LAMBDA + nc],
               coef=sc[SC_COEF:SC_COEF + nc], pl2=sc[SC_PL2])
    if a["backup_mode"]:
        out.update(breq=sc[SC_BREQ:SC_BREQ + n_cbf], blam=sc[SC_BLAMBDA:SC_BLAMBDA + n_cbf],
                   bcoef=sc[SC_BCOEF:SC_BCOEF + n_cbf], bpl2=sc[SC_BPL2])
    rho, brho = sc[SC_RHO_F64:SC_RHO_F64 + 4].copy().view(np.float64)
    return out, float(rho), float(brho)


def sc_untouched(sc, a):
    """Indices of the scalars block that the step must leave bit-identical: everything outside the write-back window
    (SC_RATIO..SC_BPL2, SC_LAMBDA..SC_MEAN_LOGP-1), and inside it whatever the step has no value for."""
    n_cbf, nc, mode = a["n_cbf"], a["n_cbf"] + a["n_clf"], a["backup_mode"]
    keep = np.ones(SC_SIZE, dtype=bool)
    keep[[SC_RATIO, SC_PL2]] = False
    keep[SC_RHO_F64:SC_RHO_F64 + 2] = False
    for base in (SC_LAMBDA, SC_COEF, SC_REQ):
        keep[base:base + nc] = False
    if mode:
        keep[SC_BPL2] = False
        for base in (SC_BLAMBDA, SC_BCOEF, SC_BREQ):
            keep[base:base + n_cbf] = False
    if mode == 2:
        keep[SC_BRHO_F64:SC_BRHO_F64 + 2] = False
    return keep


def exact_partials(n_blk, ncol, seed=21):
    """Partials that are small integers times 2^-6: every float32 sum of them is exact in any order."""
    return torch.randint(0, 64, (n_blk, ncol), generator=gen(seed + ncol)).float() / 64.0
