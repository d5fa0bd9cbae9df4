"""``odeint_dense``: ONE adaptive dopri5 solve of this build's NODE models, read at every point of a time grid —
``torchdiffeq.odeint(func, y0, t)`` with ``len(t) >= 2`` on its adaptive path (0.2.3, as the oracle restates dopri5):
the initial-step selection runs once, the error norm is taken over the whole batch tensor (one problem), steps are not
clipped at the output times, and ``out[j]`` is the 4th-order interpolant of the first accepted step that reaches
``t[j]``.  (``odeint`` serves exactly two time points; ``ode_grid.odeint_grid`` is the fixed-grid rule, euler / rk4.
A chain of ``odeint`` calls restarted at every grid point is another solution: the initial-step selection runs again at
every point and steps are cut there.)

How it runs.  The solver's device-driven chain (``ode_dopri``) is run to ``t[-1] - t[0]`` as it is; it leaves every
accepted step in a step slot — the stage derivatives ``K[0..6]``, the stage inputs ``Y`` — and the step sizes in
``hslots``.  One launch, ``nlbac_dopri_dense_fwd``, then walks the slots and writes all T - 1 output states.  The
backward starts with one launch, ``nlbac_dopri_dense_bwd``, that leaves in EVERY slot the gradient its outputs send to
the step's ``y0`` / ``y1`` / ``K``; then the accepted steps are differentiated last to first by the solver's step
backward WITHOUT a chain description (``nlbac_node_rk_bwd`` / ``nlbac_concat_rk_bwd`` add onto what a slot already
holds; the chain's own carry mode ignores a slot's ``dK`` / ``dy0``), with one small ``nlbac_dopri_dense_carry`` launch
between two steps for what step i + 1 sends back to step i.  That is one backward launch per accepted step, as in
``odeint``, plus one carry launch per step boundary.

``odeint_dense_adjoint`` is the same solve with the continuous adjoint as its backward (torchdiffeq's ``odeint_adjoint``
on a time grid): nothing of the forward is kept but the outputs, the carried columns and the interval lengths; the
backward walks the grid's intervals last to first, one adaptive adjoint solve each
(``ode_adjoint.AffineAdjoint.backward_adjoint_dense``), with one ``nlbac_adj_dense_restart`` launch at every grid point.

``odeint_dense(..., step_control="tile")`` is the same call with every 32-row tile of the batch an adaptive solve of its
own (the control-affine NODE at the register-resident kernels' shapes; ``ode_traj.AffineTileDense``): the rows of tile j
are ``odeint_dense`` of those rows alone.  No tile waits for another and the host never looks into the solve, so the whole
time series is ONE launch (``nlbac_node_dopri_tile_dense_fwd``: the tile emits every output behind the accepted step
that reaches it) and its backward one more (``nlbac_node_dopri_tile_dense_bwd``, + the weight-gradient launch).

Not served: decreasing ``t``, hipGraph capture of the batch-wide control (the solve needs the host's look at the control
block), and nets or settings the device-driven chain refuses — each raises, none runs some other way.
"""
import math

import torch

from . import _lib
from . import ode_traj as T
from .arena import stream_ptr
from .ode_grid import _steps_of

STEP_CONTROLS = ("batch", "tile")
TILE_MAX_STEPS = 32                        # the slots a tile gets when max_steps is None
SOLVERS_KEY = "_odeint_dense_solvers"      # on the model: {keep mode: solver}, apart from odeint's, rollout's and the grid's
ADJOINT = "adjoint"                        # the key of odeint_dense_adjoint's solver beside the keep modes


def _taus(t):
    """The grid's checks (``ode_grid._steps_of``'s); returns the output times 1 .. T-1 in solver time — the field is
    autonomous, the solve runs over [0, t[-1] - t[0]] — each ``float(t[j]) - float(t[0])``, as ``odeint`` forms its dt."""
    try:
        _steps_of(t)
    except (ValueError, TypeError) as e:
        raise type(e)(str(e).replace("odeint_grid:", "odeint_dense:")) from None
    times = [float(v) for v in torch.as_tensor(t).detach().cpu()]
    return tuple(v - times[0] for v in times[1:])


def _check_tile(func, n, step_control, max_steps, info):
    """The checks of ``step_control`` / ``max_steps`` / ``info`` (``func`` is a NeuralODEModel, ``n`` its rows); returns
    the slots a tile gets (``max_steps``, or 32), None under the batch-wide control."""
    if step_control not in STEP_CONTROLS:
        raise ValueError("odeint_dense: step_control is one of %s; got %r" % (", ".join(STEP_CONTROLS), step_control))
    if step_control == "batch":
        if max_steps is not None or info is not None:
            raise ValueError("odeint_dense: max_steps and info go with step_control='tile' (the batch-wide control keeps "
                             "its steps in the solver's slot pool and reports through the solver)")
        return None
    if info is not None and not isinstance(info, dict):
        raise ValueError("odeint_dense: info is a dict (it receives the device tensors accepted / attempts / status) or "
                         "None; got %s" % type(info).__name__)
    if max_steps is None:
        max_steps = TILE_MAX_STEPS
    if isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < 1:
        raise ValueError("odeint_dense: max_steps must be an int >= 1 (the accepted steps a tile may keep) or None (%d); "
                         "got %r" % (TILE_MAX_STEPS, max_steps))
    if max_steps * 7 * n >= 2 ** 31:
        raise ValueError("odeint_dense: max_steps * 7 stages * %d rows is 2^31 or more (the launch's limit: %d * 7 * %d); "
                         "use a smaller max_steps or fewer rows" % (n, max_steps, n))
    if not func.affine:
        raise NotImplementedError("odeint_dense: step_control='tile' serves the control-affine NODE only "
                                  "(nlbac_node_dopri_tile_ok); the single-net form is left open")
    if not T.AffineTile.shapes_ok(func):
        raise NotImplementedError("odeint_dense: step_control='tile' needs nets the register-resident kernels serve "
                                  "(nlbac_node_dopri_tile_ok: both nets 64, 100 or 128 wide, f_net five layers, g_net "
                                  "four); there is no other path under tile-local control")
    return max_steps


def _check_device(y0):
    if y0.device.type != "cuda":
        raise ValueError("odeint_dense: y0 must be on a CUDA device; got %s" % y0.device)


def _check(func, y0, t, atol, rtol, adjoint):
    """Every argument check, before anything touches a device; returns the output times (``_taus``)."""
    taus = _check_args(func, y0, t, atol, rtol, adjoint)
    _check_device(y0)
    return taus


def _check_args(func, y0, t, atol, rtol, adjoint):
    """``_check`` without its last one, the device of ``y0`` (``odeint_dense`` puts the step control's checks between)."""
    from .sac_cbf_clf.model import NeuralODEModel
    if adjoint:
        raise NotImplementedError("odeint_dense: the backward goes through the accepted steps; the continuous adjoint on "
                                  "a dense dopri5 solve is an entry of its own, odeint_dense_adjoint")
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.ode_dense.odeint_dense integrates this build's NeuralODEModel (its field runs as HIP "
                        "kernels); got %s" % type(func).__name__)
    taus = _taus(t)
    for name, v in (("atol", atol), ("rtol", rtol)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("odeint_dense: %s must be a Python number; got %s" % (name, type(v).__name__))
        if not (math.isfinite(v) and v > 0):
            raise ValueError("odeint_dense: %s must be positive and finite; got %r" % (name, v))
    if not isinstance(y0, torch.Tensor):
        raise TypeError("odeint_dense: y0 must be a tensor; got %s" % type(y0).__name__)
    if y0.dtype != torch.float32:
        raise TypeError("odeint_dense: y0 must be float32; got %s" % y0.dtype)
    width = func.n_s + (func.n_u if func.affine else func.n_carry)
    if y0.dim() != 2 or y0.shape[1] != width or y0.shape[0] < 1:
        raise ValueError("odeint_dense: y0 must be (batch, %d) = [x | carried columns]; got %s" % (width, tuple(y0.shape)))
    return taus


def solver_of(func, mode):
    """The (cached) solver of ``func``'s dense solves that keep ``mode`` (``ode_traj.keep_mode``): a solver of its own, so
    that what a long solve teaches it (``_chain_len``, the slot pool's size) stays out of ``odeint``'s."""
    svs = func.__dict__.setdefault(SOLVERS_KEY, {})
    sv = svs.get(mode)
    if sv is None:
        sv = T.traj_class(func).Solver(func, func.device_handles()[0].arena.device)
        sv.keep_acts = mode not in ("inputs", ADJOINT)      # (no grad: the same kernels as odeint's solver; nothing is read back)
        sv.interp_fold = False               # the attempt launches interpolate nothing: every output is read off the slots
        if mode == ADJOINT:
            # nothing of a step is kept (the slots are the smallest there are: no activation rows, no dz), and the values
            # are still those of the solvers that keep rows
            sv.adjoint = sv.rows_sums = True
        svs[mode] = sv
    return sv


def odeint_dense(func, y0, t, *, atol=1e-7, rtol=1e-5, adjoint=False, step_control="batch", max_steps=None, info=None):
    """The dopri5 solution of the NODE ``func`` (either form; a model owned by an agent included) at every point of the
    time grid ``t`` (1-D tensor or sequence, T >= 2 finite strictly increasing times): returns ``out`` (T, B, n_s + n_c)
    with ``out[0] = y0``, from ONE adaptive solve over ``[t[0], t[-1]]``.  ``y0`` (B, n_s + n_c) is CUDA float32,
    ``[x | carried columns]`` as ``odeint`` takes it; the carried columns are copied through to every ``out[j]``.

    The initial-step selection runs once, the error norm is the RMS over the whole batch tensor, steps are not cut at the
    output times; for j >= 1, ``out[j]`` is the 4th-order interpolant of the FIRST accepted step ``[t_i, t_i + h_i]``
    with ``t_i + h_i >= tau_j``, at ``x = (tau_j - t_i) / h_i``, where ``tau_j = float(t[j]) - float(t[0])`` (the field
    is autonomous in solver time).  ``odeint_dense(func, y0, [t0, t1])`` equals ``odeint(func, y0, [t0, t1],
    method="dopri5")`` in the values bit for bit.

    Differentiable w.r.t. ``y0`` (state and carried columns) and ``func.parameters()`` through one autograd node; ``t``
    is a constant and step sizes carry no gradient, as everywhere in this build.  The weight copies are refreshed first.
    What is kept follows what needs a gradient, as in ``rollout``; under ``torch.no_grad`` nothing beyond the solver's
    step slots.  Memory grows with the number of accepted steps, not with T.

    ``step_control="tile"`` (the control-affine NODE; ``"batch"``, the default, is everything above): every 32-row tile
    ``R_j = [32 j, min(32 j + 32, B))`` is a dense solve of its own —

        out[:, R_j] == odeint_dense(func, y0[R_j], t, atol=..., rtol=...)

    with its own initial-step selection, norms over its rows' ``[x | u]`` entries (a partial last tile is a smaller
    batch), step sizes and accept decisions.  No tile waits for another, so the whole time series is ONE launch that the
    host never looks into, its backward one more (+ the weight-gradient launch for parameter gradients), with the keep
    modes above.  When a backward follows, a tile KEEPS at most ``max_steps`` accepted steps (an int >= 1; None: 32;
    ``max_steps * 7 * B`` stays below 2^31); under ``torch.no_grad`` it is no limit.  A tile that runs out of slots, or
    takes more than 1000 attempts, writes NaN into its rows of every output it has not yet emitted and sets its status;
    the other tiles are unaffected, nothing synchronises, and ``backward()`` — which reads status and counts first, in one
    small copy — raises ``NlbacError`` naming ``max_steps`` and the largest count seen.  ``info`` (a dict) receives
    device tensors without a synchronisation: ``accepted`` and ``attempts`` (n_tiles,) int32 and ``status`` (n_tiles,)
    int32 — 0 ok, 1 no slot left, 2 attempt cap.  ``max_steps`` / ``info`` with ``"batch"`` are a ``ValueError``.

    Raises instead of running some other way: decreasing ``t`` (``ValueError``), ``adjoint=True`` (``NotImplementedError``),
    under ``"batch"`` a call inside a hipGraph capture (``RuntimeError``: the solve needs the host's look at the control
    block; the tile-local solve needs no look) and a solver whose device-driven chain is not available — nets the fused
    step kernels refuse, or ``device_loop`` off (``NotImplementedError``); under ``"tile"`` the single-net form and nets
    the register-resident kernels refuse (``NotImplementedError`` naming ``nlbac_node_dopri_tile_ok``)."""
    taus = _check_args(func, y0, t, atol, rtol, adjoint)
    slots = _check_tile(func, y0.shape[0], step_control, max_steps, info)
    _check_device(y0)
    if slots is not None:
        # the tile-local solve: no solver, no chain — the cached solvers of the batch-wide control are not touched
        params = tuple(func.parameters())
        func.refresh_device_weights()
        return _DenseTileFunction.apply(func, taus, float(atol), float(rtol), T.keep_mode(params, y0), slots, info, y0,
                                        *params)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("odeint_dense: not inside a hipGraph capture — the adaptive solve needs the host's look at the "
                           "control block to know how many steps were accepted")
    params = tuple(func.parameters())
    mode = T.keep_mode(params, y0)
    sv = solver_of(func, mode)
    if not sv._chain_ok(1, y0.shape[0]):
        raise NotImplementedError(
            "odeint_dense: needs the device-driven dopri5 chain (_chain_ok(1, %d) is false: fused=%s — the fused step "
            "kernels refuse these nets — device_loop=%s); the host-driven and stage-by-stage paths emit no interior "
            "points" % (y0.shape[0], sv.fused, sv.device_loop))
    func.refresh_device_weights()
    return _DenseFunction.apply(func, sv, taus, float(atol), float(rtol), mode, y0, *params)


class _DenseSolve:
    """What one dense solve keeps: the solver (whose step slots hold the accepted steps), the output times on the device
    and the carried columns."""

    def __init__(self, sv, taus, x0, c, atol, rtol, xs):
        n, ns = x0.shape[0], sv.n_s
        self.sv, self.n, self.n_out, self.c = sv, n, len(taus), c
        sv.forward(x0, c, 1, n, "dopri5", taus[-1], atol, rtol)
        st = sv.ctx["chain"]
        assert not st["ip"] and not sv.ctx.get("out_mapped"), "a dense solve interpolates nothing inside its attempts"
        self.solve_id = sv.stats["solves"]
        self.pool, self.hslots = st["pool"], st["ch"].hslots
        self.tau = torch.tensor(taus, dtype=torch.float64, device=x0.device)
        ws0 = self.pool.ws(n, 0)
        _lib.call("nlbac_dopri_dense_fwd", x0.data_ptr(), ws0.Y[6].data_ptr(), ws0.K.data_ptr(), self.pool.slot_floats,
                  sv._ctl(1).data_ptr(), self.hslots, self.pool.n_slots, self.tau.data_ptr(), self.n_out, n, ns,
                  xs.data_ptr(), stream_ptr())

    def backward(self, dxs, need_p):
        """dxs (T - 1, n, n_s): d loss / d out[1:] on the state columns.  Returns (dx0, dc, flat parameter gradient or
        None); dc is the solve's own share of the carried columns' gradient."""
        sv, n, pool = self.sv, self.n, self.pool
        assert sv.stats["solves"] == self.solve_id, \
            "odeint_dense: backward must run before the next odeint_dense with the same model and what it keeps"
        ctx, ns, s = sv.ctx, sv.n_s, stream_ptr()
        nacc = ctx["nacc"][0]
        wss = [pool.ws(n, i).bwd(sv) for i in range(nacc + 1)]
        ws0 = wss[0]
        _lib.call("nlbac_dopri_dense_bwd", dxs.data_ptr(), pool.slot_floats, sv._ctl(1).data_ptr(), self.hslots,
                  pool.n_slots, self.tau.data_ptr(), self.n_out, n, ns, ws0.dy0.data_ptr(), ws0.dy1.data_ptr(),
                  ws0.dK.data_ptr(), s)
        du = sv._buf("du", n, sv.n_u)
        for i in range(nacc, -1, -1):
            ws = wss[i]
            if i < nacc:
                # (a launch of the library's, not ATen ops: see the loop in AffineNodeSolver.backward)
                nxt = wss[i + 1]
                _lib.call("nlbac_dopri_dense_carry", nxt.dy0.data_ptr(), nxt.dK[0].data_ptr(), n * ns, ws.dy1.data_ptr(),
                          ws.dK[6].data_ptr(), s)
            sv._rk_fused_bwd(ws, self.c, 1, n, "dopri5", i == 0, True, need_p, None, self.hslots + 8 * i, pool.n_slots,
                             ws.dy1, du, i == nacc)
        flat = None
        if need_p:
            arena = sv.node.device_handles()[0].arena
            used = sv.accumulate_param_grads(arena, max(1, arena.n_slabs // len(ctx["steps"])))
            flat = T._reduce(arena, used)
        return ws0.dy0, du, flat


def _solve(sv, taus, atol, rtol, y0):
    """One dense solve on ``sv`` from ``y0`` (B, n_s + n_c): returns (out (T, B, n_s + n_c), the ``_DenseSolve``)."""
    n, ns = y0.shape[0], sv.n_s
    y0 = y0.detach().contiguous()
    x0, c = y0[:, :ns].contiguous(), y0[:, ns:].contiguous()
    xs = torch.empty(len(taus), n, ns, dtype=torch.float32, device=y0.device)
    solve = _DenseSolve(sv, taus, x0, c, atol, rtol, xs)
    out = torch.empty(len(taus) + 1, n, y0.shape[1], dtype=torch.float32, device=y0.device)
    out[0].copy_(y0)
    out[1:, :, :ns].copy_(xs)
    out[1:, :, ns:].copy_(c)          # (the carried columns, the same at every output point)
    return out, solve


class _DenseFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, sv, taus, atol, rtol, mode, y0, *params):
        out, solve = _solve(sv, taus, atol, rtol, y0)
        ctx.func, ctx.mode, ctx.n_params = func, mode, len(params)
        ctx.kept = solve if mode != "none" else None
        return out

    @staticmethod
    def backward(ctx, dout):
        assert ctx.kept is not None, "odeint_dense: nothing was kept for a backward (the forward ran without gradients)"
        ns = ctx.func.n_s
        dout = dout.float()
        need_p = ctx.mode == "params" and any(ctx.needs_input_grad[7:])
        dx0, dc, flat = ctx.kept.backward(dout[1:, :, :ns].contiguous(), need_p)
        gy0 = None
        if ctx.needs_input_grad[6]:
            # d/d carried columns: the solve's own, and the share of every output point they were copied to
            gy0 = dout[0] + torch.cat([dx0, dc + dout[1:, :, ns:].sum(0)], dim=1)
        gp = T.param_grads(ctx.func, flat) if need_p else [None] * ctx.n_params
        return (None, None, None, None, None, None, gy0, *gp)


class _DenseTileFunction(torch.autograd.Function):
    """``odeint_dense(step_control="tile")`` as one autograd node over ``ode_traj.AffineTileDense``."""

    @staticmethod
    def forward(ctx, func, taus, atol, rtol, mode, slots, info, y0, *params):
        n, ns = y0.shape[0], func.n_s
        y0 = y0.detach().contiguous()
        x0, c = y0[:, :ns].contiguous(), y0[:, ns:].contiguous()
        xs = torch.empty(len(taus), n, ns, dtype=torch.float32, device=y0.device)
        solve = T.AffineTileDense(func, n, taus, slots, info, mode, atol, rtol, y0.device)
        solve.forward(x0, c, xs)
        out = torch.empty(len(taus) + 1, n, y0.shape[1], dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        out[1:, :, :ns].copy_(xs)
        # the carried columns, the same at every output point; NaN with the state where a stopped tile emitted nothing
        nan = torch.isnan(xs[:, :, :1])
        out[1:, :, ns:].copy_(torch.where(nan, xs[:, :, :1], c))
        ctx.func, ctx.mode, ctx.n_params = func, mode, len(params)
        ctx.kept = solve if mode != "none" else None
        return out

    @staticmethod
    def backward(ctx, dout):
        assert ctx.kept is not None, "odeint_dense: nothing was kept for a backward (the forward ran without gradients)"
        ns = ctx.func.n_s
        dout = dout.float()
        need_p = ctx.mode == "params" and any(ctx.needs_input_grad[8:])
        dx0, dc, flat = ctx.kept.backward(dout[1:, :, :ns].contiguous(), need_p)
        gy0 = None
        if ctx.needs_input_grad[7]:
            # (_DenseFunction.backward's expression: the solve's own, and the share of every output point)
            gy0 = dout[0] + torch.cat([dx0, dc + dout[1:, :, ns:].sum(0)], dim=1)
        gp = T.param_grads(ctx.func, flat) if need_p else [None] * ctx.n_params
        return (None, None, None, None, None, None, None, gy0, *gp)


# ---------------------------------------------------------------------------------------------------------------------
# The continuous adjoint on a dense solve: torchdiffeq.odeint_adjoint(func, y0, t) with default arguments on a time grid
# ---------------------------------------------------------------------------------------------------------------------
def _lengths(t):
    """The lengths of the grid's intervals, ``float(t[j]) - float(t[j-1])`` of the entries as ``_taus`` reads them (a
    Python sequence rounded to float32 first); with two points the one length is ``_taus``'s one output time."""
    times = [float(v) for v in torch.as_tensor(t).detach().cpu()]
    return tuple(times[j] - times[j - 1] for j in range(1, len(times)))


def odeint_dense_adjoint(func, y0, t, *, atol=1e-7, rtol=1e-5, adjoint_params=None):
    """``torchdiffeq.odeint_adjoint(func, y0, t)`` (0.2.3, default arguments: dopri5, the adjoint's method and tolerances
    the forward's, the mixed adjoint norm) on a time grid: ``odeint_dense``'s arguments, checks, refusals and VALUES — the
    same single dense solve, ``out`` (T, B, n_s + n_c) bit for bit — with the backward as a second solve that keeps
    nothing of the forward but ``out`` (which the caller holds), the carried columns and the interval lengths.  Step
    slots are the solver's pool, as under ``torch.no_grad``; memory does not grow with the number of accepted steps.

    Differentiable as one autograd node w.r.t. ``y0`` and, with ``adjoint_params=None`` (every parameter of ``func``,
    torchdiffeq's default), ``func.parameters()``; ``adjoint_params=()`` leaves the parameter adjoint out of the
    augmented state and of the step-size norm.  Anything else raises ``NotImplementedError``.

    The backward is ``OdeintAdjointMethod.backward`` on the grid: the intervals [t[j-1], t[j]] are solved from j = T-1
    down to 1, each a fresh adaptive solve over its length (own initial-step selection; steps are not cut, the lower end
    is the interpolant of the last accepted step).  At a grid point the state part of the augmented state is RESET to the
    stored ``out[j]`` and ``dout[j]``'s state columns are added to the state adjoint; the state adjoint, the carried
    columns' adjoint and the parameter adjoint are CARRIED from the interval above and take part in the mixed norm, as in
    torchdiffeq.  The one deviation from torchdiffeq: the output gradients on the CARRIED columns (whose derivative is
    zero, so they pass through every interval unchanged) are added outside the solve — ``gy0[:, n_s:] = dout[0][:, n_s:] +
    a_c + sum_j dout[j][:, n_s:]`` — and stay out of the norm, as ``odeint_adjoint`` does for two points.  With two time
    points gradients and values are ``odeint_adjoint(..., method="dopri5")``'s bit for bit.  The gradient equals
    ``odeint_dense``'s direct back-propagation to solver tolerance only, and every interval costs at least one host wait
    on the control block.

    Raises as ``odeint_dense`` does (decreasing ``t``, hipGraph capture, nets the device-driven chain refuses).  Not
    offered: several problems in one solve, a sample-sharded solve, adjoint tolerances or method other than the
    forward's."""
    with_params = adjoint_params is None
    if not with_params and len(tuple(adjoint_params)) != 0:
        raise NotImplementedError("odeint_dense_adjoint: adjoint_params is None (all of func's parameters) or ()")
    taus = _check(func, y0, t, atol, rtol, False)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("odeint_dense_adjoint: not inside a hipGraph capture — the adaptive solves need the host's look "
                           "at the control block to know how many steps were accepted")
    sv = solver_of(func, ADJOINT)
    if not sv._chain_ok(1, y0.shape[0]):
        raise NotImplementedError(
            "odeint_dense_adjoint: needs the device-driven dopri5 chain (_chain_ok(1, %d) is false: fused=%s — the fused "
            "step kernels refuse these nets — device_loop=%s); the host-driven and stage-by-stage paths emit no interior "
            "points" % (y0.shape[0], sv.fused, sv.device_loop))
    func.refresh_device_weights()
    return _DenseAdjointFunction.apply(func, sv, taus, _lengths(t), float(atol), float(rtol), with_params, y0,
                                       *func.parameters())


class _DenseAdjointFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, sv, taus, lengths, atol, rtol, with_params, y0, *params):
        out, solve = _solve(sv, taus, atol, rtol, y0)
        # kept: the carried columns and the lengths; the step slots stay the pool's, the output times go with `solve`
        ctx.func, ctx.sv, ctx.c, ctx.lengths, ctx.solve_id = func, sv, solve.c, lengths, solve.solve_id
        ctx.with_params, ctx.n_params = with_params, len(params)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        sv, ns = ctx.sv, ctx.func.n_s
        assert sv.stats["solves"] == ctx.solve_id, \
            "odeint_dense_adjoint: backward must run before the next odeint_dense_adjoint with the same model"
        out, = ctx.saved_tensors
        dout = dout.float().contiguous()
        need_p = ctx.with_params and any(ctx.needs_input_grad[8:])
        a_x, a_c, theta = sv.backward_adjoint_dense(out, dout, ctx.c, ctx.lengths, need_p)
        gy0 = None
        if ctx.needs_input_grad[7]:
            # the carried columns' output gradients never entered the solve: added here, as odeint_adjoint adds them
            gy0 = dout[0] + torch.cat([a_x, a_c + dout[1:, :, ns:].sum(0)], dim=1)
        gp = T.param_grads(ctx.func, theta.clone()) if need_p else [None] * ctx.n_params
        return (None, None, None, None, None, None, None, gy0, *gp)
