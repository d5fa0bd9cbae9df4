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
from .ode_grid import _check_y0, _steps_of
from .ode_node import PackedSolve, SolveNode, _reduce

STEP_CONTROLS = ("batch", "tile")
TILE_MAX_STEPS = 32                        # the slots a tile gets when max_steps is None
SOLVERS_KEY = "_odeint_dense_solvers"      # on the model: {keep mode: solver}, apart from odeint's, rollout's and the grid's
ADJOINT = "adjoint"                        # the key of odeint_dense_adjoint's solver beside the keep modes


def _taus(t):
    """The grid's checks (``ode_grid._steps_of``'s); returns the output times 1 .. T-1 in solver time — the field is
    autonomous, the solve runs over [0, t[-1] - t[0]] — each ``float(t[j]) - float(t[0])``, as ``odeint`` forms its dt."""
    _steps_of(t, "odeint_dense")
    times = [float(v) for v in torch.as_tensor(t).detach().cpu()]
    return tuple(v - times[0] for v in times[1:])


def _check_tile(func, n, step_control, max_steps, info, tile_steps=None):
    """The checks of ``step_control`` / ``max_steps`` / ``info`` / ``tile_steps`` (``func`` is a NeuralODEModel, ``n`` its
    rows); returns the slots a tile gets (``max_steps``, or 32), None under the batch-wide control — and, where
    ``tile_steps`` counts them per tile, ``ode_traj.tile_steps_arg``'s form of it."""
    if step_control not in STEP_CONTROLS:
        raise ValueError("odeint_dense: step_control is one of %s; got %r" % (", ".join(STEP_CONTROLS), step_control))
    if step_control == "batch":
        if max_steps is not None or info is not None or tile_steps is not None:
            raise ValueError("odeint_dense: max_steps, tile_steps and info go with step_control='tile' (the batch-wide "
                             "control keeps its steps in the solver's slot pool and reports through the solver)")
        return None
    if info is not None and not isinstance(info, dict):
        raise ValueError("odeint_dense: info is a dict (it receives the device tensors accepted / attempts / status) or "
                         "None; got %s" % type(info).__name__)
    if tile_steps is not None:
        if max_steps is not None:
            raise ValueError("odeint_dense: tile_steps (a slot count per tile) and max_steps (one for all tiles) exclude "
                             "each other; got both")
        T.check_tile_steps("odeint_dense", tile_steps, n, 1, "a solve keeps at least one step")
    else:
        if max_steps is None:
            max_steps = TILE_MAX_STEPS
        if isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < 1:
            raise ValueError("odeint_dense: max_steps must be an int >= 1 (the accepted steps a tile may keep) or None "
                             "(%d); got %r" % (TILE_MAX_STEPS, max_steps))
        if max_steps * 7 * n >= 2 ** 31:
            raise ValueError("odeint_dense: max_steps * 7 stages * %d rows is 2^31 or more (the launch's limit: %d * 7 * "
                             "%d); use a smaller max_steps or fewer rows" % (n, max_steps, n))
    if not func.affine:
        raise NotImplementedError("odeint_dense: step_control='tile' serves the control-affine NODE only "
                                  "(nlbac_node_dopri_tile_ok); the single-net form is left open")
    if not T.AffineTile.shapes_ok(func):
        raise NotImplementedError("odeint_dense: step_control='tile' needs nets the register-resident kernels serve "
                                  "(nlbac_node_dopri_tile_ok: both nets 64, 100 or 128 wide, f_net five layers, g_net "
                                  "four); there is no other path under tile-local control")
    return max_steps if tile_steps is None else T.tile_steps_arg(tile_steps)


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
    _check_y0("odeint_dense", func, y0)
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


def odeint_dense(func, y0, t, *, atol=1e-7, rtol=1e-5, adjoint=False, step_control="batch", max_steps=None, info=None,
                 tile_steps=None):
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

    ``tile_steps`` (with ``"tile"`` only, in place of ``max_steps``: both is a ``ValueError``) counts the slots PER TILE,
    as in ``rollout``: a sequence of ints or a 1-D integer CPU tensor, one entry >= 1 per tile (``ceil(B / 32)``; a CUDA
    tensor is a ``ValueError`` asking for ``.cpu()``), gives tile j exactly ``tile_steps[j]`` slots.  The kept buffers
    hold ``sum(tile_steps)`` pages of 7 stages x 32 rows, not ``max_steps * n_tiles`` — per page, with n_g = n_s n_u:
    input gradients 224 (4 n_g + 112) bytes; parameter gradients 224 (4 n_g + 4 n_s + 28 hid + 112) forward and
    224 (4 n_g + 4 n_s + 28 hid) more in the backward — and the weight-gradient launch walks ``sum * 7 * 32`` rows
    (``>= 2**31``: a ``ValueError``).  Values and input gradients are those of a ``max_steps`` call that suffices, bit
    for bit; parameter gradients to summation order.  A tile that needs more than its own count stops as above, and
    the backward's ``NlbacError`` names ``tile_steps`` and that tile's count.  ``tile_steps="count"``: the forward launch
    runs once with nothing kept (the same kernel instance, hence the same steps), the tiles' counts come to the host,
    and the kept forward runs with exactly those — ONE EXTRA FORWARD LAUNCH AND ONE HOST WAIT per call; under
    ``torch.no_grad()`` nothing is kept and nothing is counted.  ``info`` also receives ``slots``: the int32 CPU tensor
    of per-tile counts the buffers were sized with, to pass back in on the next call over similar inputs.

    Raises instead of running some other way: decreasing ``t`` (``ValueError``), ``adjoint=True`` (``NotImplementedError``),
    under ``"batch"`` a call inside a hipGraph capture (``RuntimeError``: the solve needs the host's look at the control
    block; the tile-local solve needs no look) and a solver whose device-driven chain is not available — nets the fused
    step kernels refuse, or ``device_loop`` off (``NotImplementedError``); under ``"tile"`` the single-net form and nets
    the register-resident kernels refuse (``NotImplementedError`` naming ``nlbac_node_dopri_tile_ok``)."""
    taus = _check_args(func, y0, t, atol, rtol, adjoint)
    slots = _check_tile(func, y0.shape[0], step_control, max_steps, info, tile_steps)
    _check_device(y0)
    if slots is not None:
        # the tile-local solve: no solver, no chain — the cached solvers of the batch-wide control are not touched
        params = tuple(func.parameters())
        func.refresh_device_weights()
        mode = T.keep_mode(params, y0)
        if tile_steps is None:
            solve = _DenseTileSolve(func, taus, float(atol), float(rtol), mode, slots, info)
        else:      # (the slots are counted per tile: ``slots`` is tile_steps as the solve takes it)
            solve = _DenseTileSolve(func, taus, float(atol), float(rtol), mode, None, info, slots)
        return SolveNode.apply(solve, 1, y0, *params)
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
    return SolveNode.apply(_DenseSolve(func, sv, taus, float(atol), float(rtol), mode), 1, y0, *params)


def _dense_fwd(sv, taus, x0, c, atol, rtol, xs):
    """One dense solve on ``sv`` from ``x0`` under the carried columns ``c`` into ``xs`` (T - 1, n, n_s): the chain to
    ``taus[-1]``, then the launch that reads every output off the step slots.  Returns (the solve's id, the slot pool,
    the steps' sizes, the output times on the device)."""
    n = x0.shape[0]
    sv.forward(x0, c, 1, n, "dopri5", taus[-1], atol, rtol)
    st = sv.ctx["chain"]
    assert not st["ip"] and not sv.ctx.get("out_mapped"), "a dense solve interpolates nothing inside its attempts"
    pool, hslots = st["pool"], st["ch"].hslots
    tau = torch.tensor(taus, dtype=torch.float64, device=x0.device)
    ws0 = pool.ws(n, 0)
    _lib.call("nlbac_dopri_dense_fwd", x0.data_ptr(), ws0.Y[6].data_ptr(), ws0.K.data_ptr(), pool.slot_floats,
              sv._ctl(1).data_ptr(), hslots, pool.n_slots, tau.data_ptr(), len(taus), n, sv.n_s, xs.data_ptr(),
              stream_ptr())
    return sv.stats["solves"], pool, hslots, tau


class _DenseSolve(PackedSolve):
    """One dense solve as ``ode_node.SolveNode``'s solve.  What it keeps: the solver (whose step slots hold the accepted
    steps), the output times on the device and the carried columns."""
    api = "odeint_dense"

    def __init__(self, func, sv, taus, atol, rtol, mode):
        PackedSolve.__init__(self, func)
        self.sv, self.taus, self.tol, self.mode = sv, taus, (atol, rtol), mode
        self.n_out, self.with_params = len(taus), mode == "params"

    def solve(self, x0, c, xs):
        self.n, self.c = x0.shape[0], c
        self.solve_id, self.pool, self.hslots, self.tau = _dense_fwd(self.sv, self.taus, x0, c, *self.tol, xs)
        self.kept = self.sv if self.mode != "none" else None

    def backward(self, dout, need_in, need_p):
        """Returns (d/dy0 or None, the flat parameter gradient or None)."""
        sv, n, pool, ns = self.sv, self.n, self.pool, self.ns
        assert sv.stats["solves"] == self.solve_id, \
            "odeint_dense: backward must run before the next odeint_dense with the same model and what it keeps"
        dxs = dout[1:, :, :ns].contiguous()      # d loss / d out[1:] on the state columns
        ctx, s = sv.ctx, stream_ptr()
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
            flat = _reduce(arena, sv.accumulate_param_grads(arena, max(1, arena.n_slabs // len(ctx["steps"]))))
        if not need_in[0]:
            return None, flat
        # d/d carried columns: the solve's own (du), and the share of every output point they were copied to
        return self.grad_y0(dout, ws0.dy0, du, dout[1:, :, ns:].sum(0), self), flat


class _DenseTileSolve(PackedSolve):
    """``odeint_dense(step_control="tile")`` as ``ode_node.SolveNode``'s solve: ``ode_traj.AffineTileDense`` behind the
    packed layout."""
    api = "odeint_dense"

    def __init__(self, func, taus, atol, rtol, mode, slots, info, tile_steps=None):
        """``slots``: every tile's (``max_steps``), or None with ``tile_steps`` (``ode_traj.tile_steps_arg``'s)."""
        PackedSolve.__init__(self, func)
        self.taus, self.tol, self.mode, self.slots, self.info = taus, (atol, rtol), mode, slots, info
        self.tile_steps = tile_steps
        self.n_out, self.with_params = len(taus), mode == "params"

    def solve(self, x0, c, xs):
        tile = T.AffineTileDense(self.func, x0.shape[0], self.taus, self.slots, self.info, self.mode, *self.tol, x0.device,
                                 self.tile_steps)
        tile.forward(x0, c, xs)
        self.kept = tile if self.mode != "none" else None

    def carried(self, xs, c):
        # the same at every output point; NaN with the state where a stopped tile emitted nothing
        nan = torch.isnan(xs[:, :, :1])
        return torch.where(nan, xs[:, :, :1], c)

    def backward(self, dout, need_in, need_p):
        ns = self.ns
        dx0, dc, flat = self.kept.backward(dout[1:, :, :ns].contiguous(), need_p)
        if not need_in[0]:
            return None, flat
        return self.grad_y0(dout, dx0, dc, dout[1:, :, ns:].sum(0), self.kept), flat


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
    solve = _DenseAdjointSolve(func, sv, taus, _lengths(t), float(atol), float(rtol), with_params)
    return SolveNode.apply(solve, 1, y0, *func.parameters())


class _DenseAdjointSolve(PackedSolve):
    """``odeint_dense_adjoint`` as ``ode_node.SolveNode``'s solve: ``odeint_dense``'s forward; kept are the carried
    columns and the lengths — the step slots stay the pool's, the output times go with the forward."""
    api, saves_out = "odeint_dense_adjoint", True

    def __init__(self, func, sv, taus, lengths, atol, rtol, with_params):
        PackedSolve.__init__(self, func)
        self.sv, self.taus, self.lengths, self.tol, self.with_params = sv, taus, lengths, (atol, rtol), with_params
        self.n_out = len(taus)

    def solve(self, x0, c, xs):
        self.solve_id = _dense_fwd(self.sv, self.taus, x0, c, *self.tol, xs)[0]
        self.kept = self.c = c

    def backward(self, dout, need_in, need_p, out):
        sv, ns = self.sv, self.ns
        assert sv.stats["solves"] == self.solve_id, \
            "odeint_dense_adjoint: backward must run before the next odeint_dense_adjoint with the same model"
        dout = dout.contiguous()
        a_x, a_c, theta = sv.backward_adjoint_dense(out, dout, self.c, self.lengths, need_p)
        # the carried columns' output gradients never entered the solve: added here, as odeint_adjoint adds them
        gy0 = self.grad_y0(dout, a_x, a_c, dout[1:, :, ns:].sum(0), self) if need_in[0] else None
        return gy0, theta.clone() if need_p else None
