"""Float64 references, shared cases and the comparator for the update's loss heads: the squashed-Gaussian sample and
its backward, the TD / Lyapunov targets, the ``min(Q1, Q2)`` branch terms with the alpha scalars, and the one-step MSE.
They exist as per-row entry points of ``csrc/agent_kernels.hip`` and as heads fused into the MLP launches
(``csrc/dy_heads.h``).  Imports without a GPU.

References.  One plain torch function per operation, written in the original's own form (``GaussianPolicy.sample``,
``update_parameters``) and run in the dtype of the tensors it is handed: float64 is the reference, float32 the same
formulas at the kernels' precision (what fixes ``K``).  Tensor inputs are the float32 tensors the device gets, cast up;
scalars the ABI takes as ``float`` are rounded (``T.f32``).  Every backward is ``torch.autograd.grad`` of the forward.

Decisions are read off the float32 inputs and held while the bar perturbs the values: whether a raw ``log_std`` lies
inside ``[-20, 2]`` (``inside_of``; inclusive, as ``torch.clamp`` passes its gradient and as ``in_range`` of
``gauss_bwd_one`` does) and whether ``Q1 == Q2`` (``ties_of``; both sides then move together).  A perturbation models the
rounding of a value; it must not turn a boundary row into an ordinary one, or the bar there would be as wide as the
gradient itself and no wrong boundary rule could leave it.

Comparator.  ``task_kernels_common``'s rule: an element may differ from the float64 reference by at most

    bar = K * ( max over 8 seeded draws of |f64(perturbed) - f64| + 2^-24 |f64| )

with every element of every tensor input multiplied by 1 + d, d ~ U[-2^-23, 2^-23].  The Gaussian head cancels on two
STORED float32 intermediates, exactly as the original's float32 PyTorch does: ``x - mean`` with ``x = mean + eps std``
(``std`` tiny next to ``|mean|``: the difference is rounding noise), and ``1 - y^2`` with ``y = tanh(x)`` (float32
``tanh`` is exactly 1 from ``|x|`` near 9; ``log(scale (1 - y^2) + 1e-6)`` moves by about 0.03).  No float32 code can
meet a bar that perturbs the inputs alone there, so ``reference_and_bar_noisy`` also hands the reference multiplicative
noise of the same distribution for ``x`` and ``y`` (the perturbed ``y`` clamped to [-1, 1]); the backward sees them as
float32 autograd does: the gradient of a stored value is the identity's, ``tanh'`` is formed from the stored output.

``K`` comes from the reference alone: the smallest power of two for which the float32 evaluation of the same reference,
on the CPU, stays within HALF the bar on every shared case (``test_heads_host.py`` asserts it).  It is never adjusted
from a device result.  So that a wide bar cannot hide a failure, an element whose bar exceeds ``ILL`` = 1e-4 of its
tensor's scale (max |reference|) counts as ill-conditioned: ``action``, every ``dq`` and every TD target have none;
``logp`` and ``dheads`` at most a quarter (rows saturated in ``tanh``, and the few rows that keep an O(1) mean beside a
``log_std`` near -20; the other rows that low have mean 0, so that ``x - mean`` is exact).  Where the float32 reference
is itself within 1e-5 of a tensor's scale, the GPU tests also hold that tensor to ``common.vec_close(..., 1e-4)``
(``f32_is_tight``).

``K`` and the worst float32-reference / bar ratio (CPU), then the worst device / bar ratio (MI355X), per operation:

    operation                K   float32 reference   device
    gauss_fwd                8   0.258               0.292
    gauss_bwd                4   0.410               0.346
    td_targets               8   0.251               0.177
    td_value                 4   0.404               0.321
    actor_q                  2   0.496               0.496
    actor_losses             4   0.425               0.256
    actor_scalars            2   0.407               0.280
    alpha_refresh            1   0.226               0.444
    mse                      2   0.374               0.422

(``actor_losses``: the scalars of ``actor_scalars`` formed from the rows themselves, as a launch that sums its own rows
leaves them.  The device column is the worst over the per-row entry points and the three families of fused launches;
for the fused forward the reference's inputs are the heads the launch itself wrote.)
"""
import functools
import math

import numpy as np
import torch

import task_kernels_common as T
from task_kernels_common import F32, F64, ROWS, SENTINEL, bar_ratio, f32, gen, run   # noqa: F401  (shared with the tests)

DRAWS = T.DRAWS
ILL = 1e-4
LOG_SIG_MIN, LOG_SIG_MAX, SAMPLE_EPS, MAX_NU = -20.0, 2.0, 1e-6, 4
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))

# operation -> K (the table above)
K = {"gauss_fwd": 8, "gauss_bwd": 4, "td_targets": 8, "td_value": 4, "actor_q": 2, "actor_losses": 4, "actor_scalars": 2, "alpha_refresh": 1,
     "mse": 2}

# the scalars block (csrc/scalars.h)
SC_SIZE, SC_ALPHA, SC_PL1, SC_BPL1, SC_ALOSS, SC_BALOSS, SC_MEAN_LOGP, SC_MEAN_BLOGP = 128, 0, 10, 11, 12, 13, 116, 117


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
class _Stored(torch.autograd.Function):
    """v -> v * factor with the identity's gradient: the rounding of a stored intermediate."""

    @staticmethod
    def forward(ctx, v, factor):
        return v * factor

    @staticmethod
    def backward(ctx, g):
        return g, None


class _StoredTanh(torch.autograd.Function):
    """y = clamp(tanh(x) * factor, -1, 1); the derivative is formed from the stored y, as autograd's ``tanh`` does — here
    as the same ``1 - y * y`` the forward's logarithm takes, whatever the dtype (torch's own float32 ``tanh`` backward
    fuses the product and so rounds ``1 - y^2`` differently from the forward: 5e-5 apart at |x| = 4)."""

    @staticmethod
    def forward(ctx, x, factor):
        y = torch.clamp(torch.tanh(x) * factor, -1.0, 1.0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * (1 - y * y), None


def inside_of(heads, n_u):
    """Which raw log_std of the float32 ``heads`` (n, 2 n_u) pass the clamp's gradient: -20 <= v <= 2, inclusive."""
    ls = heads[:, n_u:2 * n_u]
    return (ls >= LOG_SIG_MIN) & (ls <= LOG_SIG_MAX)


def _clamped_log_std(raw, inside):
    """clamp(raw, -20, 2) with the gradient 1 where ``inside`` (a constant mask) and 0 elsewhere."""
    c = torch.clamp(raw, LOG_SIG_MIN, LOG_SIG_MAX)
    if inside is None:
        return c
    return torch.where(inside, raw + (c - raw).detach(), c.detach())


def gauss_fwd(t, n_u, inside=None):
    """``GaussianPolicy.sample`` with the caller's eps.  heads (n, 2 n_u) = [mean | log_std], eps (n, n_u), scale, bias
    (n_u); optional ``noise_x`` / ``noise_y`` (n, n_u): the factors 1 + d of the two stored intermediates."""
    heads = t["heads"]
    mean = heads[:, :n_u]
    log_std = _clamped_log_std(heads[:, n_u:2 * n_u], inside)
    std = log_std.exp()
    x = mean + t["eps"] * std
    if "noise_x" in t:
        x = _Stored.apply(x, t["noise_x"])
    y = _StoredTanh.apply(x, t["noise_y"] if "noise_y" in t else torch.ones_like(x))
    action = y * t["scale"] + t["bias"]
    var = std * std
    # Normal(mean, std).log_prob(x).  Under the reparameterisation x - mean = eps std, so -(x - mean)^2 / (2 var) is the
    # constant -eps^2 / 2 and hands no gradient on: autograd would send eps / std * d logp to d mean through x and take it
    # off again through -mean (5e8 times the gradient itself at log_std = -20), and eps^2 d logp twice over to d log_std.
    # The value keeps the original's cancellation on the stored x (test_heads_host.py checks the gradient against plain
    # autograd where float64 can carry the cancellation).
    quad = (-((x - mean) ** 2) / (2 * var)).detach()
    logp = quad - std.log() - LOG_SQRT_2PI
    logp = logp - torch.log(t["scale"] * (1 - y * y) + SAMPLE_EPS)
    return dict(action=action, logp=logp.sum(1))


def gauss_x(t, n_u):
    """The pre-tanh sample x = mean + eps std of the float32 inputs, in float64."""
    heads = t["heads"].double()
    return heads[:, :n_u] + t["eps"].double() * torch.clamp(heads[:, n_u:2 * n_u], LOG_SIG_MIN, LOG_SIG_MAX).exp()


GAUSS_NOISE = ("noise_x", "noise_y")


def gauss_bwd(t, n_u, rows_per_problem, dlogp_mul, inside):
    """d heads of sum(da * action) + sum_i dlp_i logp_i; da = the sum of the sources ``da0`` .. ``da2`` (each (n, >= n_u),
    those present), dlp_i = alpha[i // rows_per_problem] * dlogp_mul."""
    heads = t["heads"].detach().clone().requires_grad_(True)
    n = heads.shape[0]
    out = gauss_fwd(dict(t, heads=heads), n_u, inside)
    da = torch.zeros_like(out["action"])
    for k in range(3):
        if "da%d" % k in t:
            da = da + t["da%d" % k][:, :n_u]
    dlp = t["alpha"][torch.arange(n) // rows_per_problem] * dlogp_mul
    g, = torch.autograd.grad((da * out["action"]).sum() + (dlp * out["logp"]).sum(), heads)
    return dict(dheads=g)


def td_targets(t, gamma, B_norm, mul):
    """sac_cbf_clf.py:231-246.  q1t, q2t, lt, nlogp, reward, constraint, mask, q1, q2, lf (B), alpha (1)."""
    mq = torch.min(t["q1t"], t["q2t"]) - t["alpha"][0] * t["nlogp"]
    next_q = t["reward"] + t["mask"] * gamma * mq
    next_l = t["constraint"] + t["mask"] * gamma * t["lt"]
    e = torch.stack([t["q1"] - next_q, t["q2"] - next_q, t["lf"] - next_l], 1)
    return dict(next_q=next_q, next_l=next_l, dq=2 * e / B_norm, e2=e * e, losses=(e * e).sum(0) * mul)


def td_value(t, gamma, B_norm, mul):
    """NU/sac_cbf_clf/sac_cbf_clf.py:224-233: the fourth net.  next_target, signal, mask, pred (B)."""
    y = t["signal"] + t["mask"] * gamma * t["next_target"]
    e = t["pred"] - y
    return dict(next_out=y, dpred=2 * e / B_norm, e2=e * e, loss=(e * e).sum() * mul)


def ties_of(q1, q2):
    """Rows of the float32 inputs with Q1 == Q2 (+0.0 == -0.0 among them)."""
    return q1 == q2


def actor_q(t, B, B_norm, P, ties):
    """sac_cbf_clf.py:258-273.  q1, q2, logp (P B), alpha (P): dq through ``torch.min`` (a tie hands half of -1 / B_norm
    to each side) and terms (P B, 2) = (alpha_p logp - min q, logp), whose sums the scalars are made of."""
    a = t["q1"].detach().clone().requires_grad_(True)
    b = torch.where(ties, t["q1"], t["q2"]).detach().clone().requires_grad_(True)
    m = torch.min(a, b)
    da, db = torch.autograd.grad(-(m.sum()) / B_norm, (a, b))
    alpha = t["alpha"][torch.arange(P * B) // B]
    terms = torch.stack([alpha * t["logp"] - m.detach(), t["logp"]], 1)
    return dict(dq1=da, dq2=db, terms=terms)


def actor_scalars(t, B, first, P, target_entropy):
    """sac_cbf_clf.py:292-308 on the partial sums.  partials (2, n_blk, 2), log_alpha (P): problems first .. first+P-1."""
    s = t["partials"][first:first + P].sum(1)
    pl1, mean_logp = s[:, 0] / B, s[:, 1] / B
    la = t["log_alpha"].detach().clone().requires_grad_(True)
    aloss = -(la * (mean_logp + target_entropy))              # -(log_alpha * (logp + H)).mean()
    g, = torch.autograd.grad(aloss.sum(), la)
    return dict(pl1=pl1, aloss=aloss.detach(), mean_logp=mean_logp, g_log_alpha=g)


def actor_losses(t, B, B_norm, P, ties, target_entropy):
    """The scalars of ``actor_scalars`` straight from the rows (what a launch that sums its own rows leaves): q1, q2, logp
    (P B), alpha, log_alpha (P)."""
    sums = actor_q(t, B, B_norm, P, ties)["terms"].view(P, B, 2).sum(1)
    return actor_scalars(dict(partials=sums[:, None, :], log_alpha=t["log_alpha"]), B_norm, 0, P, target_entropy)


def alpha_refresh(t):
    return dict(alpha=t["log_alpha"].exp())


def mse(t, n_norm):
    """nn.MSELoss('mean') over (n, d) with the mean's row count n_norm: dpred, and the rows' squared-error sums."""
    e = t["pred"] - t["target"]
    return dict(dpred=2 * e / (n_norm * e.shape[1]), e2=(e * e).sum(1))


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def reference_and_bar_noisy(op, fn, inputs, noise=None, seed=0, k=None):
    """``T.reference_and_bar`` with the stored intermediates perturbed together with the inputs.  ``noise``: name ->
    shape of the factor tensors (1 + d, same distribution) that the perturbed runs of ``fn`` find among their inputs;
    the reference itself runs without them."""
    k = K[op] if k is None else k
    base = run(fn, inputs, F64)
    dev = {n: torch.zeros_like(v) for n, v in base.items()}
    g = gen(1000 + seed)
    factor = lambda shape: 1.0 + (torch.rand(shape, generator=g, dtype=F64) * 2 - 1) * 2.0 ** -23
    for _ in range(DRAWS):
        nud = {n: v.double() * factor(v.shape) for n, v in inputs.items()}
        for n, shape in (noise or {}).items():
            nud[n] = factor(shape)
        out = run(fn, nud, F64)
        dev = {n: torch.maximum(dev[n], (out[n] - base[n]).abs()) for n in base}
    return base, {n: k * (dev[n] + 2.0 ** -24 * base[n].abs()) for n in base}


def ill_share(ref, bar):
    """Share of the elements whose bar exceeds ``ILL`` of the tensor's scale."""
    scale = max(float(ref.abs().max()), 1e-30)
    return float((bar > ILL * scale).double().mean()) if ref.numel() else 0.0


def f32_is_tight(fn, inputs, ref, name):
    """Is the float32 evaluation of the reference within 1e-5 of the tensor's scale everywhere?  (Then the GPU tests
    also apply ``vec_close(..., 1e-4)``.)"""
    got = run(fn, inputs, F32)[name].double()
    scale = max(float(ref[name].abs().max()), 1e-30)
    return bool(torch.isfinite(got).all()) and float((got - ref[name]).abs().max()) <= 1e-5 * scale


def block_sums(v, block=256):
    return T.block_sums(v if v.dim() > 1 else v[:, None], block)


# ---------------------------------------------------------------------------
# shared cases (float32 tensors; built once, read unchanged)
# ---------------------------------------------------------------------------
GAMMA = f32(0.99)
TARGET_ENTROPY = f32(-2.0)
ALPHAS = (0.2, 0.0625 * 11)           # two problems, different temperatures
PER_REGIME = 8
# the Gaussian head's regimes, per row (every component of the row): name -> (raw log_std or None, mean kind)
GAUSS_REGIMES = ("plain", "min", "max", "below_min", "above_max", "far_below", "far_above", "saturated", "eps0",
                 "min_with_mean")
NEXT_BELOW_MIN = float(np.nextafter(np.float32(LOG_SIG_MIN), np.float32(-np.inf)))
NEXT_ABOVE_MAX = float(np.nextafter(np.float32(LOG_SIG_MAX), np.float32(np.inf)))


def gauss_regime_rows(n):
    """Row -> index into ``GAUSS_REGIMES``: row 0 and most rows plain; where n allows, ``PER_REGIME`` rows of every other
    regime, interleaved from row 1 on."""
    reg = np.zeros(n, dtype=np.int64)
    special = len(GAUSS_REGIMES) - 1
    k = min(PER_REGIME * special, max(n - 1, 0))
    reg[1:1 + k] = 1 + np.arange(k) % special
    return reg


@functools.lru_cache(maxsize=None)
def gauss_case(n, n_u, seed=1):
    """heads (n, 2 n_u), eps (n, n_u), scale in [0.5, 2], bias != 0 — and the rows' regimes.  Plain rows: mean N(0, 1),
    log_std N(-1, 0.5^2).  The rows with log_std at or below -20 have mean exactly 0 (``x - mean`` is exact) except the
    few of ``min_with_mean``; ``saturated``: |mean| in [4, 12] with std e^-3, so |x| runs from 4 to 12."""
    g = gen(seed + 31 * n + 7 * n_u)
    reg = gauss_regime_rows(n)
    mean = T.randn(g, n, n_u)
    ls = T.randn(g, n, n_u) * 0.5 - 1.0
    eps = T.randn(g, n, n_u)
    sat = (4.0 + 8.0 * T.rand(g, n, n_u)) * torch.where(T.rand(g, n, n_u) < 0.5, -1.0, 1.0)
    name = lambda r: GAUSS_REGIMES[r]
    for i in range(n):
        r = name(reg[i])
        if r in ("min", "min_with_mean"):
            ls[i] = LOG_SIG_MIN
        elif r == "max":
            ls[i] = LOG_SIG_MAX
        elif r == "below_min":
            ls[i] = NEXT_BELOW_MIN
        elif r == "above_max":
            ls[i] = NEXT_ABOVE_MAX
        elif r == "far_below":
            ls[i] = -60.0
        elif r == "far_above":
            ls[i] = 15.0
        elif r == "saturated":
            ls[i], mean[i] = -3.0, sat[i]
        elif r == "eps0":
            eps[i] = 0.0
        if r in ("min", "below_min", "far_below"):
            mean[i] = 0.0
    # |x| from 4 to 12 in even steps over the saturated rows' first component: tanhf just below 1 and exactly +-1
    rows = np.nonzero(reg == GAUSS_REGIMES.index("saturated"))[0]
    for j, i in enumerate(rows):
        mean[i, 0] = (4.0 + 8.0 * j / max(len(rows) - 1, 1)) * (1.0 if j % 2 else -1.0)
    t = dict(heads=torch.cat((mean, ls), 1), eps=eps, scale=0.5 + 1.5 * T.rand(g, n_u),
             bias=(0.25 + T.rand(g, n_u)) * torch.where(T.rand(g, n_u) < 0.5, -1.0, 1.0))
    return t, reg


def gauss_noise(t):
    return {k: tuple(t["eps"].shape) for k in GAUSS_NOISE}


# (n_u, sources of d action, problems, B_norm / B)
GAUSS_BWD_VARIANTS = ((1, 0, 1, 1), (2, 1, 2, 2), (3, 3, 2, 1), (4, 3, 1, 2))


@functools.lru_cache(maxsize=None)
def gauss_bwd_case(B, n_u, n_src, P, seed=2):
    """The forward's tensors on n = P B rows plus alpha (P) and ``n_src`` sources of d action, source k (n, n_u + 1 + k)
    (its own leading dimension; the columns past n_u are never read)."""
    n = P * B
    t, reg = gauss_case(n, n_u, seed)
    g = gen(seed + 13 * n + n_src)
    t = dict(t, alpha=torch.tensor(ALPHAS[:P], dtype=F32))
    for k in range(n_src):
        t["da%d" % k] = T.randn(g, n, n_u + 1 + k)
    return t, reg


def heads_regimes_of(heads, eps, n_u):
    """For heads that a launch produced (test B): per element, is log_std on a boundary / outside, |x| beyond 4."""
    ls = heads[:, n_u:2 * n_u]
    x = heads[:, :n_u].double() + eps.double() * torch.clamp(ls, LOG_SIG_MIN, LOG_SIG_MAX).double().exp()
    return dict(at_min=ls == LOG_SIG_MIN, at_max=ls == LOG_SIG_MAX, outside=(ls < LOG_SIG_MIN) | (ls > LOG_SIG_MAX),
                big_x=x.abs() > 4)


RCM_LD, RCM_COLS = 6, dict(reward=0, constraint=2, mask=5)


@functools.lru_cache(maxsize=None)
def td_case(B, seed=3):
    """The TD head's inputs; ``rcm`` (B, 6) holds reward / constraint / mask as columns 0 / 2 / 5 of one row-major block.
    A third of the rows have mask 0, every fifth row q1t == q2t, |nlogp| up to 50.  Also the fourth net's
    (``td_value``): next_target xt, its signal in column 3 of ``rcm``, pred xq."""
    g = gen(seed + 17 * B)
    t = {k: T.randn(g, B) * 3 for k in ("q1t", "q2t", "lt", "q1", "q2", "lf", "xt", "xq")}
    i = torch.arange(B)
    t["q2t"] = torch.where(i % 5 == 1, t["q1t"], t["q2t"])
    t["nlogp"] = (T.rand(g, B) * 2 - 1) * 50
    rcm = T.randn(g, B, RCM_LD)
    rcm[:, RCM_COLS["mask"]] = (i % 3 != 0).float()
    t["rcm"] = rcm
    t["alpha"] = torch.tensor([ALPHAS[0]], dtype=F32)
    return t


def td_inputs(t):
    """The reference's inputs of ``td_targets`` out of a ``td_case``: the columns of the block as vectors."""
    out = {k: t[k] for k in ("q1t", "q2t", "lt", "nlogp", "q1", "q2", "lf", "alpha")}
    out.update({k: t["rcm"][:, c].contiguous() for k, c in RCM_COLS.items()})
    return out


XSIG_COL = 3


def td_value_inputs(t):
    return dict(next_target=t["xt"], signal=t["rcm"][:, XSIG_COL].contiguous(),
                mask=t["rcm"][:, RCM_COLS["mask"]].contiguous(), pred=t["xq"])


ACTOR_ROW_KINDS = ("a<b", "b<a", "a==b", "+0,-0", "-0,+0")


def actor_row_kinds(n):
    """Row -> index into ``ACTOR_ROW_KINDS``: a third each of a < b, b < a and a == b, and where n allows ``PER_REGIME``
    rows of each pairing of signed zeros."""
    kind = np.arange(n) % 3
    k = min(2 * PER_REGIME, max(n - 3, 0))
    kind[3:3 + k] = 3 + np.arange(k) % 2
    return kind


@functools.lru_cache(maxsize=None)
def actor_case(B, P, seed=4):
    """q1, q2, logp (P B) and alpha (P)."""
    n = P * B
    g = gen(seed + 19 * B + P)
    kind = actor_row_kinds(n)
    q1 = T.randn(g, n) * 3
    gap = T.rand(g, n) + 2.0 ** -10
    q2 = q1.clone()
    k = torch.from_numpy(kind)
    q2 = torch.where(k == 0, q1 + gap, q2)
    q2 = torch.where(k == 1, q1 - gap, q2)
    q1 = torch.where(k == 3, torch.tensor(0.0), q1)
    q2 = torch.where(k == 3, torch.tensor(-0.0), q2)
    q1 = torch.where(k == 4, torch.tensor(-0.0), q1)
    q2 = torch.where(k == 4, torch.tensor(0.0), q2)
    return dict(q1=q1, q2=q2, logp=T.randn(g, n) * 5, alpha=torch.tensor(ALPHAS[:P], dtype=F32)), kind


LOG_ALPHA_STRIDE = 3


@functools.lru_cache(maxsize=None)
def scalars_case(n_blk, seed=5):
    """partials (2, n_blk, 2) of both problems and log_alpha (2)."""
    g = gen(seed + n_blk)
    return dict(partials=T.randn(g, 2, n_blk, 2) * 40, log_alpha=torch.tensor([-1.25, 0.4375]) + 0.1 * T.randn(g, 2))


def sc_block(seed=9):
    """A scalars block (float32, 128) of sentinels."""
    return torch.randn(SC_SIZE, generator=gen(seed)) * 100


def sc_slots(first, P):
    """name -> indices of the scalars block that ``actor_scalars_one`` writes for problems first .. first + P - 1."""
    pick = lambda a, b: [(a, b)[p] for p in range(first, first + P)]
    return dict(pl1=pick(SC_PL1, SC_BPL1), aloss=pick(SC_ALOSS, SC_BALOSS), mean_logp=pick(SC_MEAN_LOGP, SC_MEAN_BLOGP))


MSE_SHAPES = ((1, 0, 1), (3, 2, 2), (10, 1, 1))       # (d, extra leading-dimension columns, n_norm / n)


@functools.lru_cache(maxsize=None)
def mse_case(n, d, seed=6):
    g = gen(seed + 23 * n + d)
    pred = T.randn(g, n, d) * 2
    return dict(pred=pred, target=pred + 0.3 * T.randn(g, n, d))


# ---------------------------------------------------------------------------
# every (operation, case) the float32 reference is held to half the bar on
# ---------------------------------------------------------------------------
def gauss_bwd_setup(B, n_u, n_src, P, norm_mul):
    """(fn, inputs, noise, B_norm, dlogp_mul) of one backward variant on the shared case."""
    t, _ = gauss_bwd_case(B, n_u, n_src, P)
    B_norm = norm_mul * B
    mul = f32(1.0 / B_norm)
    inside = inside_of(t["heads"], n_u)
    return (lambda q: gauss_bwd(q, n_u, B, mul, inside)), t, gauss_noise(t), B_norm, mul


def actor_losses_setup(B, P):
    """(fn, inputs, B_norm) of ``actor_losses`` on the shared rows and the shared log_alpha."""
    t, _ = actor_case(B, P)
    t = dict(t, log_alpha=scalars_case(1)["log_alpha"][:P].clone())
    ties = ties_of(t["q1"], t["q2"])
    B_norm = P * B
    return (lambda q: actor_losses(q, B, B_norm, P, ties, TARGET_ENTROPY)), t, B_norm


def actor_q_setup(B, P):
    """(fn, inputs, B_norm): one problem normalises by B, two by 2 B."""
    t, _ = actor_case(B, P)
    ties = ties_of(t["q1"], t["q2"])
    B_norm = P * B
    return (lambda q: actor_q(q, B, B_norm, P, ties)), t, B_norm


SCALARS_VARIANTS = ((0, 1), (1, 1), (0, 2))           # (first_problem, P)


def scalars_inputs(n_blk, first, P):
    t = scalars_case(n_blk)
    return dict(partials=t["partials"], log_alpha=t["log_alpha"][first:first + P].clone())


# the fused heads (csrc/dy_heads.h): below, at and just past a 16- and a 32-row tile, 7 tiles, 38 / 19 tiles (a second group
# of the two-level election); MANY_TILES = 257 tiles of 16 rows (elected_tile_sums' stride of 256)
HEAD_BATCHES = (1, 15, 16, 17, 31, 33, 100, 600)
MANY_TILES = 4112
GAUSS_HEAD_VARIANTS = ((2, 1, 1, 1), (2, 3, 2, 2))      # one net, two nets: (n_u, sources, problems, B_norm / B)


def head_norm_mul(B):
    """B_norm / B of the TD head's cases: B for the odd batch sizes, 2 B for the even ones."""
    return 1 if B % 2 else 2


def shared_cases():
    """[(operation, label, fn, inputs, noise or None)]"""
    out = []
    for B in HEAD_BATCHES + (MANY_TILES,):
        norm_mul = head_norm_mul(B) if B != MANY_TILES else 1
        a = (norm_mul * B, f32(1.0 / (norm_mul * B)))
        out.append(("td_targets", "head B%d norm%d" % (B, norm_mul), lambda q, a=a: td_targets(q, GAMMA, *a),
                    td_inputs(td_case(B)), None))
        out.append(("td_value", "head B%d norm%d" % (B, norm_mul), lambda q, a=a: td_value(q, GAMMA, *a),
                    td_value_inputs(td_case(B)), None))
        if B == MANY_TILES:
            continue
        for n_u, n_src, P, norm_mul in GAUSS_HEAD_VARIANTS:
            fn, t, noise, _, _ = gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
            out.append(("gauss_bwd", "head B%d nu%d src%d P%d norm%d" % (B, n_u, n_src, P, norm_mul), fn, t, noise))
        for P in (1, 2):
            fn, t, _ = actor_q_setup(B, P)
            out.append(("actor_q", "head B%d P%d" % (B, P), fn, t, None))
            fn, t, _ = actor_losses_setup(B, P)
            out.append(("actor_losses", "head B%d P%d" % (B, P), fn, t, None))
    for B in ROWS:
        for n_u in range(1, MAX_NU + 1):
            t, _ = gauss_case(B, n_u)
            out.append(("gauss_fwd", "B%d nu%d" % (B, n_u), lambda q, n_u=n_u: gauss_fwd(q, n_u), t, gauss_noise(t)))
        for n_u, n_src, P, norm_mul in GAUSS_BWD_VARIANTS:
            fn, t, noise, _, _ = gauss_bwd_setup(B, n_u, n_src, P, norm_mul)
            out.append(("gauss_bwd", "B%d nu%d src%d P%d norm%d" % (B, n_u, n_src, P, norm_mul), fn, t, noise))
        for norm_mul in (1, 2):
            B_norm = norm_mul * B
            mul = f32(1.0 / B_norm)
            out.append(("td_targets", "B%d norm%d" % (B, norm_mul),
                        lambda q, a=(B_norm, mul): td_targets(q, GAMMA, *a), td_inputs(td_case(B)), None))
            out.append(("td_value", "B%d norm%d" % (B, norm_mul),
                        lambda q, a=(B_norm, mul): td_value(q, GAMMA, *a), td_value_inputs(td_case(B)), None))
        for P in (1, 2):
            fn, t, _ = actor_q_setup(B, P)
            out.append(("actor_q", "B%d P%d" % (B, P), fn, t, None))
            fn, t, _ = actor_losses_setup(B, P)
            out.append(("actor_losses", "B%d P%d" % (B, P), fn, t, None))
        for d, _, norm_mul in MSE_SHAPES:
            out.append(("mse", "n%d d%d norm%d" % (B, d, norm_mul), lambda q, m=norm_mul * B: mse(q, m), mse_case(B, d), None))
    for n_blk in (1, 3):
        for first, P in SCALARS_VARIANTS:
            t = scalars_inputs(n_blk, first, P)
            out.append(("actor_scalars", "blk%d first%d P%d" % (n_blk, first, P),
                        lambda q, a=(first, P): actor_scalars(q, 256.0 * n_blk, *a, TARGET_ENTROPY), t, None))
            out.append(("alpha_refresh", "blk%d first%d P%d" % (n_blk, first, P),
                        lambda q: alpha_refresh(dict(log_alpha=q["log_alpha"])), t, None))
    return out
