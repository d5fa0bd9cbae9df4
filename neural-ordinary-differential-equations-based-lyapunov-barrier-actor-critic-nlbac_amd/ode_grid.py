"""``odeint_grid``: the solution of this build's NODE models at every point of a time grid, euler / rk4 —
``torchdiffeq.odeint(func, y0, t)`` for ``len(t) >= 2`` under the fixed-grid rule without ``step_size``: one RK step per
grid interval.  (``odeint`` itself serves exactly two time points, the only call the reference makes.)

Two paths, same results, as in ``rollout``:
  * one launch (either NODE form at its register-resident kernels' shapes): the whole grid is one
    ``nlbac_node_rk_grid_fwd`` / ``nlbac_concat_rk_grid_fwd`` launch, its backward one ``nlbac_node_rk_grid_bwd`` /
    ``nlbac_concat_rk_grid_bwd`` launch (+ the weight-gradient launch over all H * stages * rows when parameter
    gradients are wanted).  They are the trajectory kernels of ``rollout`` with a step size per interval and one set of
    carried columns for all intervals, whose gradient is summed over the intervals inside the launch;
  * chained (nets wider than 128, shapes the register-resident kernels refuse): H one-interval solves on the existing
    solvers, one solver per interval when a backward follows, cached on the model under a key of their own.
``rollout.ONE_LAUNCH = False`` (env ``NLBAC_ROLLOUT_ONE_LAUNCH=0``) runs the chained path everywhere: the A/B baseline.
"""
import ctypes as C
import math

import torch

from . import ode_traj as T
from . import rollout

METHODS = ("euler", "rk4")


def _steps_of(t):
    """The grid's checks; returns the intervals' step sizes as float32 values, each formed exactly as ``odeint`` forms
    its own: the difference of the two Python floats, then the C float argument."""
    tt = torch.as_tensor(t).detach()
    if tt.dim() != 1 or tt.numel() < 2:
        raise ValueError("odeint_grid: t must be 1-D with at least two time points; got shape %s" % (tuple(tt.shape),))
    if tt.is_complex() or tt.dtype == torch.bool:
        raise TypeError("odeint_grid: t must hold real numbers; got %s" % tt.dtype)
    times = [float(v) for v in tt.cpu()]
    if not all(math.isfinite(v) for v in times):
        raise ValueError("odeint_grid: t must be finite; got %r" % (times,))
    if all(b < a for a, b in zip(times, times[1:])):
        raise ValueError("odeint_grid: t is decreasing; integrating backwards in time is out of scope here "
                         "(t must be strictly increasing)")
    if not all(b > a for a, b in zip(times, times[1:])):
        raise ValueError("odeint_grid: t must be strictly increasing (no repeated points); got %r" % (times,))
    hs = [C.c_float(b - a).value for a, b in zip(times, times[1:])]
    if not all(math.isfinite(h) and h > 0.0 for h in hs):
        raise ValueError("odeint_grid: every grid interval must be a positive finite float32; got %r" % (hs,))
    return tuple(hs)


def _steps(func, y0, t, method):
    """Every argument check, before anything touches a device; returns the intervals' step sizes (``_steps_of``)."""
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.ode_grid.odeint_grid integrates this build's NeuralODEModel (its field runs as HIP "
                        "kernels); got %s" % type(func).__name__)
    if method == "dopri5":
        raise NotImplementedError(
            "odeint_grid: dopri5 on a time grid is ONE adaptive solve over [t[0], t[-1]] whose interior points are "
            "interpolated from the accepted steps, not a chain of solves restarted at every grid point; the step driver "
            "(ode_dopri.py) does not emit interior points yet.  Use method='euler' or 'rk4', or odeint per interval")
    if method not in METHODS:
        raise ValueError("odeint_grid: method is one of %s; got %r" % (", ".join(METHODS), method))
    hs = _steps_of(t)
    if not isinstance(y0, torch.Tensor):
        raise TypeError("odeint_grid: y0 must be a tensor; got %s" % type(y0).__name__)
    if y0.dtype != torch.float32:
        raise TypeError("odeint_grid: y0 must be float32; got %s" % y0.dtype)
    width = func.n_s + (func.n_u if func.affine else func.n_carry)
    if y0.dim() != 2 or y0.shape[1] != width or y0.shape[0] < 1:
        raise ValueError("odeint_grid: y0 must be (batch, %d) = [x | carried columns]; got %s" % (width, tuple(y0.shape)))
    if y0.device.type != "cuda":
        raise ValueError("odeint_grid: y0 must be on a CUDA device; got %s" % y0.device)
    return hs


def odeint_grid(func, y0, t, *, method="rk4"):
    """The solution of the NODE ``func`` (either form; a model owned by an agent included) at every point of the time
    grid ``t`` (1-D tensor or sequence, T >= 2 finite strictly increasing times): returns ``out`` (T, B, n_s + n_c) with
    ``out[0] = y0`` and

        out[k+1] = odeint(func, out[k], t[k:k+2], method=method)[-1]

    bit for bit — one ``'euler'`` / ``'rk4'`` step per grid interval (torchdiffeq's fixed-grid rule without
    ``step_size``), the interval's step formed as ``odeint`` forms it.  ``y0`` (B, n_s + n_c) is CUDA float32,
    ``[x | carried columns]`` as ``odeint`` takes it; the carried columns (the action, or SimulatedCars' [u | t]) are
    the same over all intervals and are copied through to every ``out[k]``.

    ``'dopri5'`` raises ``NotImplementedError``: on a grid it is one adaptive solve interpolated at the interior points,
    which the step driver does not offer yet; it is not approximated by restarting at every grid point.

    Differentiable w.r.t. ``y0`` (state and carried columns) and ``func.parameters()`` through one autograd node for the
    whole grid; ``t`` is a constant (no gradient w.r.t. the times).  The weight copies are refreshed first, as in
    ``odeint``.  What is kept for the backward follows what needs a gradient, as in ``rollout``: nothing under
    ``torch.no_grad``, ReLU mask words for input gradients only, activation rows as well for parameter gradients
    (memory grows linearly with T; see ``rollout`` on the last bits of the values under input gradients only)."""
    hs = _steps(func, y0, t, method)
    params = tuple(func.parameters())
    mode = T.keep_mode(params, y0)
    func.refresh_device_weights()
    return _GridFunction.apply(func, method, hs, mode, y0, *params)


class _GridFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, method, hs, mode, y0, *params):
        H, n, ns = len(hs), y0.shape[0], func.n_s
        y0 = y0.detach().contiguous()
        x0, c = y0[:, :ns].contiguous(), y0[:, ns:].contiguous()
        dev = y0.device
        xs = torch.empty(H, n, ns, dtype=torch.float32, device=dev)        # the states behind each interval
        ctx.func, ctx.mode, ctx.n_params = func, mode, len(params)
        ctx.kept = T.solve(func, T.GridSteps(hs, dev), method, mode, rollout._one_launch_ok(func, method), x0, c, xs)
        out = torch.empty(H + 1, n, y0.shape[1], dtype=torch.float32, device=dev)
        out[0].copy_(y0)
        out[1:, :, :ns].copy_(xs)
        out[1:, :, ns:].copy_(c)          # (the carried columns, the same at every grid point)
        return out

    @staticmethod
    def backward(ctx, dout):
        assert ctx.kept is not None, "odeint_grid: nothing was kept for a backward (the forward ran without gradients)"
        ns = ctx.func.n_s
        dout = dout.float()
        need_p = ctx.mode == "params" and any(ctx.needs_input_grad[5:])
        dx0, dc, flat = ctx.kept.backward(dout[:, :, :ns].contiguous(), need_p)
        gy0 = None
        if ctx.needs_input_grad[4]:
            # d/d carried columns: out[0]'s share, then per interval its control gradient (summed k = H-1 .. 0 by the
            # backward) and out[k+1]'s share
            gy0 = torch.cat([dx0, dout[0][:, ns:] + (dc + dout[1:, :, ns:].sum(0))], dim=1)
        gp = T.param_grads(ctx.func, flat) if need_p else [None] * ctx.n_params
        return (None, None, None, None, gy0, *gp)
