"""Exact and float64 references, shared cases and the ``K`` table for the optimiser step, the streaming helpers and the
device-side draw: ``csrc/optim_kernels.hip`` (Adam, slab sum, Polyak update, scatter tables, temperature refresh,
mirror, ``nlbac_reduce_slabs`` .. ``nlbac_gather_rows``) and ``csrc/philox.h`` (``sample_rows_body``: Philox tags 0
and 1).  Imports without a GPU.

Adam.  ``adam`` is one plain torch function, run in the dtype it is handed, in the arithmetic of ``torch.optim.Adam``
single-tensor mode as ``adam_one`` writes it:

    g = slab 0 + slab 1 + ...                        (slab order)
    m += (g - m) f32(1 - 0.9)
    v  = v f32(0.999) + (f32(1 - 0.999) g) g
    p += (-step_size m) / (sqrt(v) / bc2_sqrt + f32(1e-8))
    target = target (1 - tau) + p tau                (1 - tau formed in float32)

Every slab is an input of its own, so the comparator perturbs each read and the bar follows a cancelling slab sum.
``step_size`` and ``bc2_sqrt`` are the float32 values of the state block: on the device the ones read back after the
launch, on the host ``step_consts`` (Python doubles, rounded once).  The padding of a slab (``slab_stride > n``) is NaN:
a kernel that read ``n`` where it should read ``slab_stride``, or the other way round, shows at once.

Comparator (``task_kernels_common.reference_and_bar`` with ``k=1``, scaled per output by ``K``).  An element may differ
from the float64 reference by at most

    bar = K * ( max over 8 seeded draws of |f64(x (1 + d)) - f64(x)| + 2^-24 |f64(x)| ),   d ~ U[-2^-23, 2^-23]

``K`` comes from the reference alone: the smallest power of two for which the float32 evaluation of the same reference
stays within HALF the bar on every case below (``test_optim_kernels_host.py`` asserts it).  It is never adjusted from a
device result.  Every tensor also meets ``common.vec_close(..., 1e-4)``.

Transcendentals.  The refreshed temperature is ``expf`` of the float32 parameter, an exact input: bar
``K 2^-24 |exp p|`` against the float64 ``exp``.  The policy noise is held to the float64 evaluation of its formula with
``u01`` and ``f32(6.283185307179586)`` as exact inputs: bar ``K 2^-24 (|x| + r (1 + 2 pi u))``, the rounding of the
result plus the rounding of the angle.  Both ``K`` are fitted as above, on a numpy float32 evaluation.

The draw, restated from ``test_env_reset_host.philox4x32_10``:

    key               (seed & 0xffffffff, seed >> 32)
    row of row r      (x src_rows) >> 32,  x the first word at counter (draw lo, draw hi, r, 0)     (Python integers)
    noise of quad t   (x, y, z, w) at counter (draw lo, draw hi, t, 1):
                      eps[4t .. 4t+3] = (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1),
                      r0 = sqrt(-2 log u01(x)), a0 = f32(6.283185307179586) u01(y);  r1, a1 likewise from z, w
    u01(x)            f32(x >> 8) 2^-24 + 2^-25 in float32: it lies in (0, 1] - at x >> 8 == 0xFFFFFF the sum is the tie
                      1 - 2^-25, which rounds to even, 1.0; the radius is then 0 and the noise 0, not NaN

``K`` and the worst float32-reference / bar ratio (CPU), then the worst device / bar ratio (MI355X), per operation:

    operation                K   float32 reference   device
    adam_p                   4   0.254               0.254
    adam_m                   8   0.304               0.296
    adam_v                   8   0.280               0.280
    adam_target              2   0.462               0.462
    axpby                    4   0.321               0.231
    soft_update              4   0.279               0.279
    exp                      8   0.355               0.107
    noise                    4   0.280               0.280

(Where the two columns agree, the device rounds the worst element exactly as the float32 reference does.  ``exp``: numpy's
float32 ``exp`` is further from the float64 one than the device's ``expf``.)

Not testable from outside: the mirror copy skips the entries the step refreshes because their value is written twice, by
the refreshing thread and - were they not skipped - by the last workgroup from ``mirror_src``, which is the refreshed
float itself.  The two writes differ only if the last workgroup does not yet see the refreshing thread's store; on an
MI355X it always did, so a kernel that ignores the skip passes ``test_alpha_refresh_and_mirror``.
"""
import functools
import math
import types

import numpy as np
import torch

import task_kernels_common as T
from task_kernels_common import F32, F64, f32, gen
from test_env_reset_host import philox4x32_10

# operation -> K (the table above)
K = {"adam_p": 4, "adam_m": 8, "adam_v": 8, "adam_target": 2, "axpby": 4, "soft_update": 4, "exp": 8, "noise": 4}

SENT = T.SENTINEL
LR = 4e-4
TAU = f32(0.005)
GRID = 2048 * 256                         # lanes of a full streaming grid: one more element takes a second trip

ADAM_N = (1, 3, 4, 5, 7, 1023, 1028, 4 * 256 * 3 + 6)   # tail only; float4 only; both; several workgroups
ADAM_SLABS = (1, 2, 4, 5, 8, 9)           # the unrolled trip of slab_sum4 runs 0, 1, 2 times, with and without a remainder
ADAM_PADS = (0, 8)                        # slab_stride = n rounded up to 4, plus this
ADAM_STEPS = (1, 2, 1000, 10 ** 6)
ADAM_MAGS = (1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e12)
ADAM_BIG_N = GRID * 4 + 4 * 256 + 3       # the grid-stride trip of the float4 loops, and a tail


def round4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
def step_consts(lr, t):
    """(step_size, bc2_sqrt) of step ``t`` as the state block holds them: Python doubles, rounded to float32 once."""
    return f32(lr / (1.0 - 0.9 ** t)), f32(math.sqrt(1.0 - 0.999 ** t))


def one_minus(tau):
    """``1.0f - tau`` as the kernels form it."""
    return float(np.float32(1.0) - np.float32(tau))


def adam(t, step_size, bc2_sqrt, tau=None):
    """g0 .. g{k-1}, p, m, v [, target] (n) -> p, m, v [, target] after one step."""
    g, s = t["g0"], 1
    while "g%d" % s in t:
        g, s = g + t["g%d" % s], s + 1
    m = t["m"] + (g - t["m"]) * f32(1.0 - 0.9)
    v = t["v"] * f32(0.999) + (f32(1.0 - 0.999) * g) * g
    denom = torch.sqrt(v) / torch.tensor(bc2_sqrt, dtype=v.dtype) + f32(1e-8)
    p = t["p"] + (-step_size * m) / denom
    out = dict(p=p, m=m, v=v)
    if tau is not None:
        out["target"] = t["target"] * one_minus(tau) + p * f32(tau)
    return out


@functools.lru_cache(maxsize=None)
def adam_case(n, n_slabs, pad, t, mag, cancel=False):
    """Step ``t`` on ``n`` parameters from ``n_slabs`` slabs ``round4(n) + pad`` apart, gradients of size ``mag``.
    Moments are zero at step 1 and random (of the gradients' size) otherwise; ``cancel``: slab 1 is about minus slab 0."""
    stride = round4(n) + pad
    g = gen(17 + n + 31 * n_slabs + 7 * pad + (t % 1013) + int(cancel))
    grad = torch.full((n_slabs, stride), float("nan"), dtype=F32)
    grad[:, :n] = (torch.randn(n_slabs, n, generator=g, dtype=F64) * mag).float()
    if cancel:
        grad[1, :n] = (-grad[0, :n].double() * (1.0 + 1e-3 * torch.randn(n, generator=g, dtype=F64))).float()
    if t == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = (torch.randn(n, generator=g, dtype=F64) * 0.3 * mag).float()
        v = (torch.rand(n, generator=g, dtype=F64) * mag * mag).float()
    inputs = {"g%d" % s: grad[s, :n].clone() for s in range(n_slabs)}
    inputs.update(p=torch.randn(n, generator=g), m=m, v=v, target=torch.randn(n, generator=g))
    label = "n %d slabs %d stride %d step %d |g| %.0e%s" % (n, n_slabs, stride, t, mag, " cancelling" if cancel else "")
    return types.SimpleNamespace(key=(n, n_slabs, pad, t, mag, cancel), label=label, n=n, n_slabs=n_slabs, stride=stride,
                                 t=t, mag=mag, grad=grad, inputs=inputs)


@functools.lru_cache(maxsize=None)
def adam_keys():
    """Every n x n_slabs x stride with the steps and magnitudes cycling through them, every step x magnitude at one
    shape, and the cancelling slabs."""
    keys, i = [], 0
    for n in ADAM_N:
        for n_slabs in ADAM_SLABS:
            for pad in ADAM_PADS:
                keys.append((n, n_slabs, pad, ADAM_STEPS[(i + i // 12) % 4], ADAM_MAGS[i % 6], False))
                i += 1
    for t in ADAM_STEPS:
        for mag in ADAM_MAGS:
            keys.append((1023, 2, 8, t, mag, False))
    keys += [(7, 9, 0, 2, 1.0, True), (1028, 2, 8, 1000, 1e-3, True), (1028, 5, 0, 1, 1e3, True),
             (ADAM_N[-1], 2, 8, 2, 1.0, True)]
    return tuple(dict.fromkeys(keys))


def adam_cases():
    return [adam_case(*k) for k in adam_keys()]


@functools.lru_cache(maxsize=None)
def adam_reference(key, step_size, bc2_sqrt, tau):
    """(float64 reference, bar at K = 1) of ``adam_case(*key)``; ``tau`` None: no target."""
    c = adam_case(*key)
    inputs = c.inputs if tau is not None else {k: v for k, v in c.inputs.items() if k != "target"}
    return T.reference_and_bar("adam", lambda t: adam(t, step_size, bc2_sqrt, tau), inputs, k=1)


def adam_float32(key, step_size, bc2_sqrt, tau):
    c = adam_case(*key)
    return T.run(lambda t: adam(t, step_size, bc2_sqrt, tau), c.inputs, F32)


def adam_big_gradient(g):
    """Step 2 on 1023 parameters with every gradient entry ``g`` (slab 0; slab 1 is zero) -> (case, grad, inputs).
    The second moment takes ``(f32(1 - 0.999) g) g``: 1e37 at g = 1e20, which float32 still holds - an ordinary case,
    held to the float64 reference - and +inf from g = 1e21 on, where the step is m / inf = 0 and p stays as it is.
    Both are the float32 formula's own results."""
    c = adam_case(1023, 2, 8, 2, 1.0)
    grad = c.grad.clone()
    grad[:, :c.n] = 0.0
    grad[0, :c.n] = g
    return c, grad, dict(c.inputs, g0=grad[0, :c.n].clone(), g1=grad[1, :c.n].clone())


def ulp_close(x, want):
    """``x`` is ``want`` or one of its two float32 neighbours."""
    w = np.float32(want)
    return np.float32(x) in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf)))


def scatter_layout(n, slots, seed=3):
    """A hand-made scatter table: (index [n, slots] into a float buffer, -1 = no slot; the buffer's length).  About a
    third of the entries are empty; every fifth parameter has exactly one slot (at a random position of its entry), every
    seventh all of them; the addressed floats lie in shuffled order among floats that nothing addresses."""
    rng = np.random.RandomState(seed + n + slots)
    used = rng.rand(n, slots) > 1.0 / 3.0
    one = np.arange(0, n, 5)
    used[one] = False
    used[one, rng.randint(0, slots, size=len(one))] = True
    used[np.arange(3, n, 7)] = True
    count = int(used.sum())
    length = count + count // 2 + 5
    index = np.full((n, slots), -1, dtype=np.int64)
    index[used] = rng.permutation(length)[:count]
    return index, length


# ---------------------------------------------------------------------------
# temperature refresh and mirror
# ---------------------------------------------------------------------------
ALPHA_N = 4 * 256 * 3 + 6
# offsets of the refreshed entries: the four lanes of a float4 of the first workgroup, the tail, another workgroup
ALPHA_OFFS = ((), (20,), (21,), (22,), (23,), (ALPHA_N - 1,), (4 * 300 + 2,), (21, ALPHA_N - 2), (4 * 300 + 3, 22))
MIRRORS = (1, 128, 1024)


def exp_reference(p_new):
    """float32 array -> (float64 exp, bar at K = 1)."""
    ref = np.exp(np.asarray(p_new, dtype=np.float32).astype(np.float64))
    return ref, 2.0 ** -24 * np.abs(ref)


def np_ratio(x, ref, bar):
    """``task_kernels_common.bar_ratio`` on numpy arrays."""
    ref = np.asarray(ref, dtype=np.float64)
    return T.bar_ratio(np.asarray(x, dtype=np.float64), torch.from_numpy(ref), torch.from_numpy(np.asarray(bar, dtype=np.float64)))


# ---------------------------------------------------------------------------
# streaming helpers
# ---------------------------------------------------------------------------
STREAM_N = (1, 255, 257, GRID + 77)       # the last takes the second grid-stride trip


def reduce_slabs(grad, n):
    """(n_slabs, stride) float32 -> the first n columns added in slab order, in float32."""
    g = grad[0, :n].copy()
    for s in range(1, grad.shape[0]):
        g = g + grad[s, :n]
    return g


def sum_partials(part, mul):
    """(n_blk, n_cols) float32 -> mul * (sequential float32 sum over the blocks): one multiply, after the sum."""
    s = np.zeros(part.shape[1], dtype=np.float32)
    for b in range(part.shape[0]):
        s = s + part[b]
    return s * np.float32(mul)


def axpby(t, a, b):
    return dict(out=a * t["x"] + b * t["y"] if "y" in t else a * t["x"])


def soft_update(t, tau):
    return dict(target=t["target"] * one_minus(tau) + t["src"] * f32(tau))


@functools.lru_cache(maxsize=None)
def stream_case(op, n, mag=1.0):
    g = gen(41 + n % 100003 + (op == "axpby"))
    r = lambda: (torch.randn(n, generator=g, dtype=F64) * mag).float()
    if op == "axpby":
        a, b = f32(0.37), f32(-1.9)
        return types.SimpleNamespace(op=op, n=n, mag=mag, a=a, b=b, inputs=dict(x=r(), y=r()), fn=lambda t: axpby(t, a, b),
                                     label="n %d |x| %.0e" % (n, mag))
    return types.SimpleNamespace(op=op, n=n, mag=mag, tau=TAU, inputs=dict(target=r(), src=r()), fn=lambda t: soft_update(t, TAU),
                                 label="n %d |x| %.0e" % (n, mag))


def stream_cases():
    return [stream_case(op, n) for op in ("axpby", "soft_update") for n in STREAM_N] + \
           [stream_case(op, 257, mag) for op in ("axpby", "soft_update") for mag in (1e-12, 1e12)]


@functools.lru_cache(maxsize=None)
def stream_reference(op, n, mag=1.0):
    c = stream_case(op, n, mag)
    return T.reference_and_bar(op, c.fn, c.inputs, k=1)


# ---------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------
M32 = 0xFFFFFFFF
PAIRS = ((5, 1), (5 + 2 ** 32, 1), (5, 1 + 2 ** 32), (0x9ABCDEF012345678, 0xFEDCBA9876543210))   # every half matters
TWO_PI = np.float32(6.283185307179586)
U01_WORDS = (0, 0xFF, 0x100, 0x7FFFFF00, 0xFFFFFF00, 0xFFFFFFFF)


def draw_words(seed, draw, count, tag):
    """The four output words (uint32 arrays of ``count``) of draw ``draw`` under ``seed`` for items 0 .. count-1."""
    return philox4x32_10((draw & M32, draw >> 32, np.arange(count), tag), (seed & M32, seed >> 32))


def row_of(x, src_rows):
    """``(x src_rows) >> 32`` in Python integers."""
    return (int(x) * int(src_rows)) >> 32


def row_indices(seed, draw, n_rows, src_rows):
    return np.array([row_of(x, src_rows) for x in draw_words(seed, draw, n_rows, 0)[0]], dtype=np.int64)


def u01(x):
    """``(float)(x >> 8) * 0x1p-24f + 0x1p-25f``, with its float32 rounding."""
    x = np.asarray(x, dtype=np.uint32)
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)


def noise_from_words(words, dtype):
    """(eps [4 q], bar at K = 1) from the four word arrays of q quads, evaluated in ``dtype``."""
    u = [u01(w).astype(dtype) for w in words]
    out, scale = [], []
    for ur, ua in ((u[0], u[1]), (u[2], u[3])):
        r = np.sqrt(dtype(-2.0) * np.log(ur))
        a = dtype(TWO_PI) * ua
        out += [r * np.cos(a), r * np.sin(a)]
        scale += [np.abs(r) * (1.0 + a)] * 2
    eps = np.stack(out, 1).reshape(-1)
    bar = 2.0 ** -24 * (np.abs(eps.astype(np.float64)) + np.stack(scale, 1).reshape(-1).astype(np.float64))
    return eps, bar


@functools.lru_cache(maxsize=None)
def noise_reference(seed, draw, n_eps):
    """(float64 noise [n_eps], bar at K = 1) of ``nlbac_sample_rows(..., n_eps, seed, draw)``."""
    eps, bar = noise_from_words(draw_words(seed, draw, (n_eps + 3) // 4, 1), np.float64)
    return eps[:n_eps], bar[:n_eps]


def noise_float32(seed, draw, n_eps):
    return noise_from_words(draw_words(seed, draw, (n_eps + 3) // 4, 1), np.float32)[0][:n_eps]


SAMPLE_SRC_ROWS = (1, 2, 3000)
SAMPLE_LD = (4, 36)
SAMPLE_ROWS = (1, 64, 300)


def sample_n_eps(n_rows, ld):
    """Noise lengths of one shape: none; ragged last quads; more and fewer noise threads than copy threads."""
    total = n_rows * ld // 4
    return (0, 1, 5, 6, 4 * (total + 300), max(1, 4 * (total // 2) - 1))


@functools.lru_cache(maxsize=None)
def sample_source(src_rows, ld):
    """(src_rows, ld) float32 rows with the row number in column 0."""
    src = torch.randn(src_rows, ld, generator=gen(5 + src_rows + ld))
    src[:, 0] = torch.arange(src_rows, dtype=F32)
    return src
