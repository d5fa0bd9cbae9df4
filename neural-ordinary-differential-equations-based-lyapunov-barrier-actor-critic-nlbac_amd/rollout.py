"""Differentiable multi-step rollouts of this build's NODE models: H env steps ahead with a new control per interval —
the chain of one-interval solves the reference builds its constraints from (C/sac_cbf_clf/sac_cbf_clf.py:437-458,
P/sac_cbf_clf/sac_cbf_clf.py:459-534: ``odeint(model, [x_k | u_k (| t_k)], [0, dt])[-1]`` per interval).

Two paths, same results:
  * one launch (either NODE form at its register-resident kernels' shapes, euler / rk4): the whole horizon is one
    ``nlbac_node_rk_traj_fwd`` launch (control-affine NODE) or one ``nlbac_concat_rk_traj_fwd`` launch (single-net
    NODE, normalised or not), its backward one ``nlbac_node_rk_traj_bwd`` / ``nlbac_concat_rk_traj_bwd`` launch (+ the
    weight-gradient launch over all H * stages * rows when parameter gradients are wanted);
  * chained (dopri5, nets wider than 128, shapes the register-resident kernels refuse): H single-interval solves on
    the existing solvers, one solver per interval, cached on the model apart from ``odeint``'s and the agent's.
``ONE_LAUNCH = False`` (env ``NLBAC_ROLLOUT_ONE_LAUNCH=0``) runs the chained path everywhere: the A/B baseline.
"""
import math
import os

import torch

from . import ode_traj as T

ONE_LAUNCH = os.environ.get("NLBAC_ROLLOUT_ONE_LAUNCH", "1") != "0"
METHODS = ("euler", "rk4", "dopri5")


def _check(func, x0, controls, dt, method):
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.rollout integrates this build's NeuralODEModel (its field runs as HIP kernels); "
                        "got %s" % type(func).__name__)
    if method not in METHODS:
        raise ValueError("rollout: method is one of %s; got %r" % (", ".join(METHODS), method))
    for name, t in (("x0", x0), ("controls", controls)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("rollout: %s must be a tensor; got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("rollout: %s must be float32; got %s" % (name, t.dtype))
    if isinstance(dt, bool) or not isinstance(dt, (int, float)):
        raise TypeError("rollout: dt must be a Python float; got %s" % type(dt).__name__)
    if not (math.isfinite(dt) and dt > 0):
        raise ValueError("rollout: dt must be a finite positive number; got %r" % (dt,))
    ns = func.n_s
    nc = func.n_u if func.affine else func.n_carry
    if x0.dim() != 2 or x0.shape[1] != ns or x0.shape[0] < 1:
        raise ValueError("rollout: x0 must be (batch, %d); got %s" % (ns, tuple(x0.shape)))
    if controls.dim() != 3 or controls.shape[0] < 1 or controls.shape[1] != x0.shape[0] or controls.shape[2] != nc:
        raise ValueError("rollout: controls must be (H >= 1, %d, %d); got %s" % (x0.shape[0], nc, tuple(controls.shape)))
    if x0.device.type != "cuda" or controls.device != x0.device:
        raise ValueError("rollout: x0 and controls must be on the same CUDA device; got %s and %s"
                         % (x0.device, controls.device))


def rollout(func, x0, controls, dt, *, method="rk4", atol=1e-7, rtol=1e-5):
    """Predict H intervals of ``dt`` ahead with the NODE ``func`` (either form; a model owned by an agent included),
    a new control per interval: returns ``out`` (H + 1, B, n_s) with ``out[0] = x0`` and

        out[k+1] = odeint(func, cat(out[k], controls[k]), tensor([0.0, dt]), method=..., atol=..., rtol=...)[-1][:, :n_s]

    ``x0`` (B, n_s) and ``controls`` (H, B, n_c) are CUDA float32; n_c is the affine form's n_u actions, or the
    single-net form's ``input_dim - n_s`` carried columns (e.g. SimulatedCars' [u | t], each interval's time column
    supplied by the caller).  ``dt`` is rounded to float32 as ``odeint``'s time grid rounds it; dopri5 starts every
    interval afresh (initial-step selection included), as H separate ``odeint`` calls do.

    Differentiable w.r.t. ``x0``, ``controls`` and ``func.parameters()`` (one autograd node for the whole horizon; the
    weight copies are refreshed first, as in ``odeint``).  What is kept for the backward follows what needs a gradient:
    nothing under ``torch.no_grad``, ReLU mask words for input gradients only, activation rows as well for parameter
    gradients — memory grows linearly with H.  The one-step kernels sum f_net's output layer in two parts when they
    keep mask words only, so a rollout differentiated w.r.t. its inputs only can differ from ``odeint``'s values in the
    last bits; without gradients, or with parameter gradients, the values are ``odeint``'s."""
    _check(func, x0, controls, dt, method)
    dt = float(torch.tensor([0.0, float(dt)], dtype=torch.float32)[1])
    params = tuple(func.parameters())
    mode = T.keep_mode(params, x0, controls)
    func.refresh_device_weights()
    return _RolloutFunction.apply(func, method, dt, float(atol), float(rtol), mode, x0, controls, *params)


def _one_launch_ok(func, method):
    return bool(ONE_LAUNCH and method in ("euler", "rk4") and T.traj_class(func).ok(func))


class _RolloutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, method, dt, atol, rtol, mode, x0, controls, *params):
        H, n, ns = controls.shape[0], x0.shape[0], func.n_s
        x0 = x0.detach().contiguous()
        u = controls.detach().contiguous()
        out = torch.empty(H + 1, n, ns, dtype=torch.float32, device=x0.device)
        first = out[0].copy_(x0)
        ctx.func, ctx.mode, ctx.n_params = func, mode, len(params)
        one = _one_launch_ok(func, method)
        # (the one launch reads x0 where the caller's tensor is; the chain's first solver keeps a reference, to out[0])
        ctx.kept = T.solve(func, T.EqualSteps(dt, H), method, mode, one, x0 if one else first, u, out.narrow(0, 1, H),
                           atol, rtol)
        return out

    @staticmethod
    def backward(ctx, dout):
        assert ctx.kept is not None, "rollout: nothing was kept for a backward (the forward ran without gradients)"
        need_p = ctx.mode == "params" and any(ctx.needs_input_grad[8:])
        dx0, du, flat = ctx.kept.backward(dout.float().contiguous(), need_p)
        gp = T.param_grads(ctx.func, flat) if need_p else [None] * ctx.n_params
        return (None, None, None, None, None, None, dx0 if ctx.needs_input_grad[6] else None,
                du if ctx.needs_input_grad[7] else None, *gp)
