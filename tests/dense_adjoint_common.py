"""The CPU reference of ``nlbac_amd.ode_dense.odeint_dense_adjoint`` and the two cases its tests share.

The forward is ``dense_common.dense_reference``.  The backward is torchdiffeq 0.2.3's ``OdeintAdjointMethod.backward`` on
a time grid, composed from the oracle's public pieces: the intervals [t[j-1], t[j]] from j = T-1 down to 1, each one
``O.odeint_tuple(G, [out[j], a] + theta_bar, L_j, "dopri5", ...)`` with ``G`` the right-hand side written in
``O._OdeintAdjoint.backward`` and ``L_j = float(t[j]) - float(t[j-1])`` of the float32 entries; the state part is reset
to the stored ``out[j]``, the adjoint ``a`` and the parameter adjoint are carried.  As on the device, the output
gradients on the CARRIED columns stay out of the solves and are added to the result.

Both cases are width-64 nets on ``dense_common``'s inputs, with shorter grids than ``dense_common``'s (two accepted
forward steps holding two outputs each) and batch-mean-loss cotangents ``randn / n`` (``test_adjoint_gpu.problem``'s
scale) drawn from the inputs' generator."""
import functools

import numpy as np
import torch

import dense_common as D
from nlbac_amd import synth
from oracle import nlbac_oracle as O

GRIDS = {"unicycle": [0.0, 0.01, 0.02, 0.05, 0.08], "cars": [0.0, 0.01, 0.03, 0.1, 0.15]}
# what the cases were chosen for: the forward's step sizes, and the attempts of every interval's adjoint solve without the
# parameter adjoint, last interval first
WANT_STEPS = {"unicycle": [0.0329, 0.0783], "cars": [0.0444, 0.2337]}
WANT_ATTEMPTS = {"unicycle": [1, 2, 1, 1], "cars": [2, 2, 1, 1]}
NAMES = ["unicycle", "cars"]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def flat(ts):
    return torch.cat([v.reshape(-1) for v in ts])


def adjoint_backward(func, params, out, dout, times, n_s, atol=1e-7, rtol=1e-5):
    """``out`` / ``dout`` (T, n, w); ``params``: the tensors of the parameter adjoint (requires_grad) or ().  Returns
    (gy0, the parameter adjoint per tensor, the step log [(h, ratio, accepted)] per interval, last interval first)."""
    params = tuple(params)

    def G(z):           # O._OdeintAdjoint.backward's right-hand side (the field is autonomous)
        yv, adj = z[0], z[1]
        with torch.enable_grad():
            yv = yv.detach().requires_grad_(True)
            fe = func(0.0, yv)
            vj = torch.autograd.grad(fe, (yv,) + params, -adj, allow_unused=True)
        vj = [torch.zeros_like(x) if v is None else v for v, x in zip(vj, (yv,) + params)]
        return [-fe.detach()] + [-v for v in vj]

    out, dout = out.detach(), dout.detach()
    a, th, logs = None, [torch.zeros_like(p) for p in params], []
    for j in range(len(times) - 1, 0, -1):
        g = dout[j].clone()
        g[:, n_s:] = 0                       # (the carried columns' output gradients are added outside the solves)
        a = g if a is None else a + g
        info = {}
        with torch.no_grad():
            z = O.odeint_tuple(G, [out[j], a] + th, times[j] - times[j - 1], "dopri5", atol, rtol, info)
        a, th = z[1], list(z[2:])
        logs.append(info["steps"])
    gy0 = dout[0] + torch.cat([a[:, :n_s], a[:, n_s:] + dout[1:, :, n_s:].sum(0)], 1)
    return gy0, th, logs


@functools.lru_cache(maxsize=None)
def case(name):
    """One case, built once: inputs, the fp32 dense forward under autograd and its DIRECT gradients under ``dout``."""
    spec = D.CASES[name]
    torch.set_num_threads(4)              # (the oracle's reduction order must not depend on what ran before)
    W = synth.agent_weights(spec["env"], 64, 0)["node"]
    y0, _, gen = spec["inputs"]()
    t = torch.tensor(GRIDS[name], dtype=torch.float32)
    dout = torch.randn(len(t), y0.shape[0], y0.shape[1], generator=gen) / y0.shape[0]
    sd = {k: torch.tensor(v, requires_grad=True) for k, v in W.items()}
    yy = y0.clone().requires_grad_(True)
    out, steps, ends = D.dense_reference(spec["node"](sd), yy, D.times_of(t))
    g = torch.autograd.grad((out * dout).sum(), [yy] + list(sd.values()))
    return dict(name=name, env=spec["env"], n_s=spec["n_s"], W=W, sd=sd, y0=y0, t=t, dout=dout, out=out.detach(),
                steps=steps, ends=ends, gy0_direct=g[0], gp_direct=flat(g[1:]))


@functools.lru_cache(maxsize=None)
def adjoint(name, with_params, two_points=False):
    """The reference adjoint of a case (``two_points``: on the grid t[[0, -1]] with the output gradients of the case's
    first and last points): dict(out, dout, t, gy0, gp (flat, or None), logs, attempts)."""
    c = case(name)
    spec = D.CASES[name]
    node = spec["node"](c["sd"])
    t, dout, out = c["t"], c["dout"], c["out"]
    if two_points:
        t, dout = t[[0, -1]], dout[[0, -1]]
        with torch.no_grad():
            out, _, _ = D.dense_reference(node, c["y0"], D.times_of(t))
    params = tuple(c["sd"].values()) if with_params else ()
    gy0, th, logs = adjoint_backward(node, params, out, dout, D.times_of(t), c["n_s"])
    return dict(out=out, dout=dout, t=t, gy0=gy0, gp=flat(th) if with_params else None, logs=logs,
                attempts=[len(s) for s in logs])
