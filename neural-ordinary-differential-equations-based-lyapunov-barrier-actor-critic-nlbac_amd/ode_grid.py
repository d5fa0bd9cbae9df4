"""``odeint_grid``: the solution of this build's NODE models at every point of a time grid, euler / rk4 —
``torchdiffeq.odeint(func, y0, t)`` for ``len(t) >= 2`` under the fixed-grid rule: one RK step per grid interval, or
(``step_size=s``, torchdiffeq's ``options=dict(step_size=s)``) steps of ``s`` on a fine grid of the solver's own from
which the output points are read off by linear interpolation (``_sub_grid`` is the rule).  (``odeint`` itself serves
exactly two time points, the only call the reference makes.)

Two paths, same results, as in ``rollout``:
  * one launch (either NODE form at its register-resident kernels' shapes): the whole grid is one
    ``nlbac_node_rk_grid_fwd`` / ``nlbac_concat_rk_grid_fwd`` launch, its backward one ``nlbac_node_rk_grid_bwd`` /
    ``nlbac_concat_rk_grid_bwd`` launch (+ the weight-gradient launch over all H * stages * rows when parameter
    gradients are wanted).  They are the trajectory kernels of ``rollout`` with a step size per interval and one set of
    carried columns for all intervals, whose gradient is summed over the intervals inside the launch; with
    ``step_size`` the ``*_subgrid_*`` twins of the four: the same kernels over the N fine intervals, which write the
    T - 1 interpolated output points instead of every interval's state and take the output gradients in between the
    intervals of the one backward launch;
  * chained (nets wider than 128, shapes the register-resident kernels refuse): H one-interval solves on the existing
    solvers, one solver per interval when a backward follows, cached on the model under a key of their own (with
    ``step_size``: per fine interval, the interpolation and its gradient as torch ops, ``ode_traj.SubGridSteps``).
``rollout.ONE_LAUNCH = False`` (env ``NLBAC_ROLLOUT_ONE_LAUNCH=0``) runs the chained path everywhere: the A/B baseline.
"""
import ctypes as C
import math

import torch

from . import ode_traj as T
from . import rollout
from .ode_node import PackedSolve, SolveNode
from .ode_consts import TABLEAU

METHODS = ("euler", "rk4")


def _steps_of(t, api="odeint_grid"):
    """The grid's checks, their messages under the entry's name ``api``; returns the intervals' step sizes as float32
    values, each formed exactly as ``odeint`` forms its own: the difference of the two Python floats, then the C float
    argument."""
    tt = torch.as_tensor(t).detach()
    if tt.dim() != 1 or tt.numel() < 2:
        raise ValueError("%s: t must be 1-D with at least two time points; got shape %s" % (api, tuple(tt.shape)))
    if tt.is_complex() or tt.dtype == torch.bool:
        raise TypeError("%s: t must hold real numbers; got %s" % (api, tt.dtype))
    times = [float(v) for v in tt.cpu()]
    if not all(math.isfinite(v) for v in times):
        raise ValueError("%s: t must be finite; got %r" % (api, times))
    if all(b < a for a, b in zip(times, times[1:])):
        raise ValueError("%s: t is decreasing; integrating backwards in time is out of scope here "
                         "(t must be strictly increasing)" % api)
    if not all(b > a for a, b in zip(times, times[1:])):
        raise ValueError("%s: t must be strictly increasing (no repeated points); got %r" % (api, times))
    hs = [C.c_float(b - a).value for a, b in zip(times, times[1:])]
    if not all(math.isfinite(h) and h > 0.0 for h in hs):
        raise ValueError("%s: every grid interval must be a positive finite float32; got %r" % (api, hs))
    return tuple(hs)


def _check_step_size(step_size):
    if isinstance(step_size, bool) or not isinstance(step_size, (int, float)):
        raise TypeError("odeint_grid: step_size must be a Python number; got %s" % type(step_size).__name__)
    if not math.isfinite(step_size) or step_size <= 0:
        raise ValueError("odeint_grid: step_size must be positive and finite; got %r" % (step_size,))
    return float(step_size)


def _sub_grid(t, step_size):
    """torchdiffeq 0.2.3's fixed-grid rule under ``options=dict(step_size=s)``, in Python floats (no device): the fine
    grid of ``_grid_constructor_from_step_size`` — ``niters = ceil((t[-1] - t[0]) / s + 1)`` points ``i s + t[0]``, the
    last one replaced by ``t[-1]`` — and where ``integrate`` reads the output points off it.  Returns

        taus   the N + 1 fine times (N = niters - 1 fine intervals),
        hs     the N fine steps as float32 values, each formed as ``_steps_of`` forms its own,
        ofs    N + 1 offsets, CSR over the outputs 1 .. T-1: interval i holds the outputs ofs[i] <= j < ofs[i+1]
               (those with taus[i+1] >= t[j] that no earlier interval took),
        theta  T - 1 weights, theta[j-1] of output j in its interval i: 1.0 when t[j] == taus[i+1], 0.0 when
               t[j] == taus[i], else the float32 of (t[j] - taus[i]) / (taus[i+1] - taus[i]):
               out[j] = y_i + theta (y_{i+1} - y_i), with y_{i+1} resp. y_i themselves at 1 resp. 0."""
    s = _check_step_size(step_size)
    _steps_of(t)                      # (the grid's own checks)
    # (a tensor's entries as _steps_of takes them; a Python sequence's numbers as they are, not rounded to float32 first:
    #  whether an output point IS a fine-grid point is decided on these values)
    tt = t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)
    times = [float(v) for v in tt.detach().cpu()]
    span = (times[-1] - times[0]) / s + 1
    if not math.isfinite(span) or span >= 2 ** 31:
        raise ValueError("odeint_grid: step_size %r cuts [%r, %r] into 2^31 fine intervals or more" % (s, times[0], times[-1]))
    niters = math.ceil(span)
    taus = [i * s + times[0] for i in range(niters)]
    taus[-1] = times[-1]
    N = niters - 1
    hs = [C.c_float(b - a).value for a, b in zip(taus, taus[1:])]
    for i, h in enumerate(hs):
        if not (math.isfinite(h) and h > 0.0):
            raise ValueError("odeint_grid: fine interval %d of %d, [%r, %r], is not a positive finite float32 step (%r): "
                             "rounding left a degenerate last interval; choose another step_size" % (i, N, taus[i], taus[i + 1], h))
    ofs, theta, j = [1], [], 1
    for i in range(N):
        t0, t1 = taus[i], taus[i + 1]
        while j < len(times) and t1 >= times[j]:
            theta.append(1.0 if times[j] == t1 else (0.0 if times[j] == t0 else C.c_float((times[j] - t0) / (t1 - t0)).value))
            j += 1
        ofs.append(j)
    assert j == len(times) and all(0.0 <= th <= 1.0 for th in theta)
    return tuple(taus), tuple(hs), tuple(ofs), tuple(theta)


def _check_y0(api, func, y0):
    """``y0`` is a float32 tensor (batch, n_s + n_c) = [x | carried columns] (``odeint_grid``'s and ``odeint_dense``'s)."""
    if not isinstance(y0, torch.Tensor):
        raise TypeError("%s: y0 must be a tensor; got %s" % (api, type(y0).__name__))
    if y0.dtype != torch.float32:
        raise TypeError("%s: y0 must be float32; got %s" % (api, y0.dtype))
    width = func.n_s + (func.n_u if func.affine else func.n_carry)
    if y0.dim() != 2 or y0.shape[1] != width or y0.shape[0] < 1:
        raise ValueError("%s: y0 must be (batch, %d) = [x | carried columns]; got %s" % (api, width, tuple(y0.shape)))


def _steps(func, y0, t, method, step_size=None):
    """Every argument check, before anything touches a device; returns the intervals: their step sizes (``_steps_of``),
    or with ``step_size`` what ``_sub_grid`` returns."""
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.ode_grid.odeint_grid integrates this build's NeuralODEModel (its field runs as HIP "
                        "kernels); got %s" % type(func).__name__)
    if method == "dopri5":
        raise NotImplementedError(
            "odeint_grid: dopri5 on a time grid is ONE adaptive solve over [t[0], t[-1]] whose interior points are "
            "interpolated from the accepted steps, not a chain of solves restarted at every grid point: that is "
            "ode_dense.odeint_dense.  Here, use method='euler' or 'rk4'")
    if method not in METHODS:
        raise ValueError("odeint_grid: method is one of %s; got %r" % (", ".join(METHODS), method))
    hs = _steps_of(t) if step_size is None else _sub_grid(t, step_size)
    _check_y0("odeint_grid", func, y0)
    if step_size is not None and len(hs[1]) * len(TABLEAU[method]["c_sol"]) * y0.shape[0] >= 2 ** 31:
        raise ValueError("odeint_grid: %d fine intervals x %d stages x %d rows is 2^31 or more (the launch's limit); "
                         "use a larger step_size or fewer rows" % (len(hs[1]), len(TABLEAU[method]["c_sol"]), y0.shape[0]))
    if y0.device.type != "cuda":
        raise ValueError("odeint_grid: y0 must be on a CUDA device; got %s" % y0.device)
    return hs


def _adjoint_steps(t, step_size):
    """Per grid interval [t[j-1], t[j]] the fine steps of its backward solve under ``adjoint=True``, in the order they are
    applied from the interval's upper end: the interval's one step (``_steps_of``), or with ``step_size`` the steps
    ``_sub_grid`` gives for [0, length] — the interval's own fine grid, anchored at its upper end."""
    if step_size is None:
        return [(h,) for h in _steps_of(t)]
    times = [float(v) for v in (t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)).detach().cpu()]
    return [_sub_grid([0.0, b - a], step_size)[1] for a, b in zip(times, times[1:])]


def odeint_grid(func, y0, t, *, method="rk4", step_size=None, adjoint=False, adjoint_chunk=None):
    """The solution of the NODE ``func`` (either form; a model owned by an agent included) at every point of the time
    grid ``t`` (1-D tensor or sequence, T >= 2 finite strictly increasing times): returns ``out`` (T, B, n_s + n_c) with
    ``out[0] = y0`` and

        out[k+1] = odeint(func, out[k], t[k:k+2], method=method)[-1]

    bit for bit — one ``'euler'`` / ``'rk4'`` step per grid interval (torchdiffeq's fixed-grid rule without
    ``step_size``), the interval's step formed as ``odeint`` forms it.  ``y0`` (B, n_s + n_c) is CUDA float32,
    ``[x | carried columns]`` as ``odeint`` takes it; the carried columns (the action, or SimulatedCars' [u | t]) are
    the same over all intervals and are copied through to every ``out[k]``.

    ``step_size=s`` (a positive finite Python number; torchdiffeq's ``options=dict(step_size=s)``): the solver steps on
    a fine grid of its own instead — ``t[0] + i s``, ending at ``t[-1]`` (``_sub_grid``) — so that the accuracy does not
    depend on where the outputs are wanted; each fine state is the one-step ``odeint`` result over its fine interval bit
    for bit, and ``out[j]`` is read off the fine interval [tau_i, tau_i+1] that holds ``t[j]``: the fine state itself
    where ``t[j]`` is a fine-grid point, else ``y_i + theta_j (y_i+1 - y_i)`` in float32, ``theta_j`` the float32 of
    ``(t[j] - tau_i) / (tau_i+1 - tau_i)``.

    ``'dopri5'`` raises ``NotImplementedError`` (with or without ``step_size``): on a grid it is one adaptive solve
    interpolated at the interior points — ``ode_dense.odeint_dense`` — and is not approximated here by restarting at
    every grid point.

    Differentiable w.r.t. ``y0`` (state and carried columns) and ``func.parameters()`` through one autograd node for the
    whole grid; ``t`` is a constant (no gradient w.r.t. the times).  The weight copies are refreshed first, as in
    ``odeint``.  What is kept for the backward follows what needs a gradient, as in ``rollout``: nothing under
    ``torch.no_grad``, ReLU mask words for input gradients only, activation rows as well for parameter gradients
    (memory grows linearly with the number of steps — T - 1, or with ``step_size`` the N fine intervals, not T: the fine
    states themselves and their gradients are never stored; see ``rollout`` on the last bits of the values under input
    gradients only).

    ``adjoint=True``: the same ``out``, differentiated by the continuous adjoint on the grid — torchdiffeq's
    ``OdeintAdjointMethod.backward``: the grid intervals are walked last to first, the state restarts at the stored
    ``out[k+1]``, the output's gradient joins the adjoint there, and every stage is re-computed; without ``step_size`` the
    autograd chain of ``odeint_adjoint`` calls over the grid intervals (bit for bit in the gradient w.r.t. ``y0``).
    Nothing is kept but ``out``.  With ``step_size`` every grid interval is solved backwards on its own fine grid,
    anchored at its upper end (``_sub_grid`` over [0, t[j] - t[j-1]]).  ``adjoint_chunk`` as in ``rollout``."""
    T.check_adjoint_chunk("odeint_grid", adjoint, adjoint_chunk)
    hs = _steps(func, y0, t, method, step_size)
    params = tuple(func.parameters())
    mode = T.keep_mode(params, y0)
    func.refresh_device_weights()
    plan = T.AdjointPlan(_adjoint_steps(t, step_size), False, adjoint_chunk, step_size is not None) if adjoint else None
    return SolveNode.apply(_GridSolve(func, method, hs, mode, plan, y0.device), 1, y0, *params)


class _GridSolve(PackedSolve):
    """One solve on a time grid as ``ode_node.SolveNode``'s solve: direct, or with an ``AdjointPlan`` the continuous
    adjoint — what is saved for the backward is then ``out`` (as a saved tensor); the carried columns are read from it."""
    api = "odeint_grid"

    def __init__(self, func, method, hs, mode, plan, device):
        PackedSolve.__init__(self, func)
        # (hs: the intervals' steps, or with step_size _sub_grid's (fine times, steps, offsets, weights))
        self.iv = T.SubGridSteps(*hs[1:], device) if isinstance(hs[0], tuple) else T.GridSteps(hs, device)
        self.n_out, self.method, self.mode, self.plan = self.iv.n_out, method, mode, plan
        self.with_params, self.saves_out = mode == "params", plan is not None

    def solve(self, x0, c, xs):
        func, one = self.func, rollout._one_launch_ok(self.func, self.method)
        if self.plan is None:
            self.kept = T.solve(func, self.iv, self.method, self.mode, one, x0, c, xs)
        else:
            self.kept = T.solve_adjoint(func, self.iv, self.method, self.mode, one, self.plan, x0, c, xs)

    def backward(self, dout, need_in, need_p, out=None):
        ns = self.ns
        dx0, dc, flat = self.kept.backward(dout[:, :, :ns].contiguous(), need_p, out=out)
        if not need_in[0]:
            return None, flat
        # d/d carried columns: out[0]'s share, then per interval its control gradient (summed k = H-1 .. 0 by the
        # backward) and every later output point's share
        return self.grad_y0(dout, dx0, dc, self.iv.sum_copied(dout[1:, :, ns:]), self.kept), flat
