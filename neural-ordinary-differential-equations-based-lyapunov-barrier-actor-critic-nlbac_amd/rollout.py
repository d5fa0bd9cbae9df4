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
dopri5 with ``step_control="tile"`` is a third: every 32-row tile under a step control of its own, the whole horizon in
one ``nlbac_node_dopri_tile_fwd`` launch and one ``nlbac_node_dopri_tile_bwd`` (``ode_traj.AffineTileDopri``).
``ONE_LAUNCH = False`` (env ``NLBAC_ROLLOUT_ONE_LAUNCH=0``) runs the chained path everywhere: the A/B baseline.

``step_size=s`` (euler / rk4) solves every control interval in steps of ``s`` with its control held — the chain of
``odeint(..., options=dict(step_size=s))`` calls, bit for bit: still one launch forward (``nlbac_node_rk_hold_fwd`` /
``nlbac_concat_rk_hold_fwd``) and one backward (``*_hold_bwd``) over the H * m fine intervals, or chained fine interval
by fine interval (``ode_traj.HeldSteps``).
"""
import math
import os

import torch

from . import ode_traj as T
from .ode_node import SolveNode

ONE_LAUNCH = os.environ.get("NLBAC_ROLLOUT_ONE_LAUNCH", "1") != "0"
METHODS = ("euler", "rk4", "dopri5")
STEP_CONTROLS = ("batch", "tile")


def _check_device(x0, controls):
    if x0.device.type != "cuda" or controls.device != x0.device:
        raise ValueError("rollout: x0 and controls must be on the same CUDA device; got %s and %s"
                         % (x0.device, controls.device))


def _check_tile(func, H, method, adjoint, step_control, max_steps, info, tile_steps=None, n=None):
    """The checks of ``step_control`` / ``max_steps`` / ``info`` / ``tile_steps`` (``n``: the rows, which ``tile_steps``
    is held against); returns the slots every tile gets (``max_steps``, or 8 H) — None under the batch-wide control and
    where ``tile_steps`` counts them per tile."""
    if step_control not in STEP_CONTROLS:
        raise ValueError("rollout: step_control is one of %s; got %r" % (", ".join(STEP_CONTROLS), step_control))
    if step_control == "batch":
        if max_steps is not None or info is not None or tile_steps is not None:
            raise ValueError("rollout: max_steps, tile_steps and info go with step_control='tile' (the batch-wide control "
                             "keeps its steps per interval and reports through the solvers)")
        return None
    if method != "dopri5":
        raise ValueError("rollout: step_control='tile' goes with method='dopri5'; %s runs on a fixed grid, which has no "
                         "step control" % method)
    if adjoint:
        raise NotImplementedError("rollout: step_control='tile' with adjoint=True is not built (the continuous adjoint "
                                  "of a tile-local solve is left open)")
    if info is not None and not isinstance(info, dict):
        raise ValueError("rollout: info is a dict (it receives the device tensors accepted / attempts / status) or None; "
                         "got %s" % type(info).__name__)
    if tile_steps is not None:
        if max_steps is not None:
            raise ValueError("rollout: tile_steps (a slot count per tile) and max_steps (one for all tiles) exclude each "
                             "other; got both")
        T.check_tile_steps("rollout", tile_steps, n, H, "every interval keeps at least one step: H = %d" % H)
    else:
        if max_steps is None:
            max_steps = 8 * H
        if isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < H:
            raise ValueError("rollout: max_steps must be an int >= H = %d (every interval keeps at least one step); got %r"
                             % (H, max_steps))
    if not func.affine:
        raise NotImplementedError("rollout: step_control='tile' serves the control-affine NODE only "
                                  "(nlbac_node_dopri_tile_ok); the single-net form is left open")
    return max_steps


def _check(func, x0, controls, dt, method, step_size=None, *, adjoint=False, step_control="batch", max_steps=None,
           info=None, tile_steps=None, on_device=True):
    """Every argument check, before anything touches a device.  Returns ``dt`` rounded to float32 as ``odeint``'s time
    grid rounds it and, with ``step_size``, the fine steps of a control interval (``ode_grid._sub_grid`` over [0, dt]).
    ``on_device=False``: everything but where the tensors are (a caller that moves them itself, afterwards)."""
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.rollout integrates this build's NeuralODEModel (its field runs as HIP kernels); "
                        "got %s" % type(func).__name__)
    if method not in METHODS:
        raise ValueError("rollout: method is one of %s; got %r" % (", ".join(METHODS), method))
    if step_size is not None and method == "dopri5":
        raise ValueError("rollout: step_size goes with method='euler' or 'rk4'; torchdiffeq's dopri5 ignores it, "
                         "which this build does not do silently")
    for name, t in (("x0", x0), ("controls", controls)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("rollout: %s must be a tensor; got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("rollout: %s must be float32; got %s" % (name, t.dtype))
    if isinstance(dt, bool) or not isinstance(dt, (int, float)):
        raise TypeError("rollout: dt must be a Python float; got %s" % type(dt).__name__)
    if not (math.isfinite(dt) and dt > 0):
        raise ValueError("rollout: dt must be a finite positive number; got %r" % (dt,))
    grid = torch.tensor([0.0, float(dt)], dtype=torch.float32)
    dt, hs = float(grid[1]), None
    if step_size is not None:
        from .ode_grid import _sub_grid      # (the one place the step_size rule lives; it imports this module)
        _, hs, _, theta = _sub_grid(grid, step_size)
        assert theta == (1.0,), "the one output of a control interval is the fine grid's end point"
    ns = func.n_s
    nc = func.n_u if func.affine else func.n_carry
    if x0.dim() != 2 or x0.shape[1] != ns or x0.shape[0] < 1:
        raise ValueError("rollout: x0 must be (batch, %d); got %s" % (ns, tuple(x0.shape)))
    if controls.dim() != 3 or controls.shape[0] < 1 or controls.shape[1] != x0.shape[0] or controls.shape[2] != nc:
        raise ValueError("rollout: controls must be (H >= 1, %d, %d); got %s" % (x0.shape[0], nc, tuple(controls.shape)))
    if hs is not None:
        from .ode_consts import TABLEAU
        H, m, S = controls.shape[0], len(hs), len(TABLEAU[method]["c_sol"])
        if H * m * S * x0.shape[0] >= 2 ** 31:
            raise ValueError("rollout: %d intervals x %d fine steps x %d stages x %d rows is 2^31 or more (the launch's "
                             "limit); use a larger step_size, a shorter horizon or fewer rows" % (H, m, S, x0.shape[0]))
    slots = _check_tile(func, controls.shape[0], method, adjoint, step_control, max_steps, info, tile_steps, x0.shape[0])
    if step_control == "tile":
        if slots is not None and slots * 7 * x0.shape[0] >= 2 ** 31:
            raise ValueError("rollout: max_steps * 7 stages * %d rows is 2^31 or more (the launch's limit: %d * 7 * %d); "
                             "use a smaller max_steps or fewer rows" % (x0.shape[0], slots, x0.shape[0]))
        if not T.AffineTileDopri.shapes_ok(func):
            raise NotImplementedError("rollout: step_control='tile' needs nets the register-resident kernels serve "
                                      "(nlbac_node_dopri_tile_ok: both nets 64, 100 or 128 wide, f_net five layers, "
                                      "g_net four); there is no chained fallback")
    if on_device:
        _check_device(x0, controls)
    return dt, hs


def rollout(func, x0, controls, dt, *, method="rk4", atol=1e-7, rtol=1e-5, step_size=None, adjoint=False,
            adjoint_chunk=None, step_control="batch", max_steps=None, info=None, tile_steps=None):
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
    last bits; without gradients, or with parameter gradients, the values are ``odeint``'s.

    ``step_size=s`` (a positive finite Python number; euler / rk4 only — with dopri5 a ``ValueError``, as in ``odeint``):
    every control interval is solved in steps of ``s`` on the fine grid ``odeint(..., options=dict(step_size=s))`` builds
    for ``[0, dt]`` (``ode_grid._sub_grid``: m steps, the last one cut at ``dt``), its control — SimulatedCars' [u | t]
    columns included — held through the interval:

        out[k+1] = odeint(func, cat(out[k], controls[k]), tensor([0.0, dt]), method=..., options=dict(step_size=s))[-1][:, :n_s]

    bit for bit, gradients w.r.t. ``x0`` and ``controls`` included.  The accuracy no longer hangs on the control rate;
    the solve is still one launch forward and one backward, over H * m fine intervals, and one autograd node.  What is
    kept grows with H * m; ``out`` and the gradients stay per control interval — the fine states and their gradients are
    never stored.  ``step_size >= dt`` gives m = 1: the results without ``step_size``.

    ``adjoint=True``: the same ``out``, differentiated by the continuous adjoint on the grid of control intervals —
    torchdiffeq's ``OdeintAdjointMethod.backward``, the autograd chain of H one-interval ``odeint_adjoint`` calls (bit
    for bit in the gradients w.r.t. ``x0`` and ``controls`` without ``step_size``; parameter gradients to summation
    order).  Nothing of the forward is kept but ``out`` itself and the controls, whatever H and ``step_size`` are: the
    backward walks the control intervals last to first, restarts the state at the stored ``out[k+1]``, and re-computes
    every stage — one launch for the whole horizon with euler / rk4 at the register-resident kernels' shapes
    (``nlbac_node_adj_traj`` / ``nlbac_concat_adj_traj``), else chained.  With ``step_size`` each control interval is
    solved backwards on its own fine grid, anchored at its upper end: the steps ``_sub_grid`` gives for [0, dt], in
    that order, so that the cut step falls at the interval's lower end.  As in ``odeint_adjoint`` the gradient equals
    the direct one only to solver accuracy, and it costs more time: every stage is evaluated again.
    ``adjoint_chunk`` (a positive int, with ``adjoint=True`` and euler / rk4 only; a ``ValueError`` otherwise): the
    backward runs in launches of that many control intervals, which changes no bit of the input gradients; with
    parameter gradients the weight-gradient batch is one chunk's stage rows, and ``None`` picks the largest chunk that
    batch admits (2^29 elements per layer) — a horizon the direct backward refuses still gets its gradients.

    ``step_control`` (dopri5's step-size control): ``"batch"``, the default, is torchdiffeq's — one RMS error norm over
    all rows, so every row takes the steps the stiffest row needs, and every attempt ends in a reduction over the batch:
    H chained solves, each a row of launches and a look by the host.  ``"tile"`` (``method="dopri5"`` on the
    control-affine NODE only) gives every 32 rows a step control of their own — the per-sample control of batched ODE
    libraries at the granularity of the kernels.  With R_j the rows [32 j, min(32 j + 32, B)):

        out[:, R_j] == rollout(func, x0[R_j], controls[:, R_j], dt, method="dopri5", atol=..., rtol=...)

    — each tile is the chain of H ``odeint`` calls on its own rows: a fresh initial-step selection per interval, norms
    over the tile's [x | u] entries (a last partial tile is a smaller batch), steps not clipped at ``dt``, ``out[k+1]``
    the interpolant at ``dt``, step sizes without a gradient.  The results differ from ``"batch"``'s within the
    tolerances.  No tile waits for another, so the whole horizon is ONE launch (``nlbac_node_dopri_tile_fwd``) that the
    host never looks into, its backward one more (``nlbac_node_dopri_tile_bwd``, + the weight-gradient launch for
    parameter gradients): one autograd node, differentiable w.r.t. ``x0``, ``controls`` and the parameters, with the
    keep modes above.  It needs nets the register-resident kernels serve (``nlbac_node_dopri_tile_ok``; a
    ``NotImplementedError`` otherwise): there is no chained fallback, and ``ONE_LAUNCH`` does not apply.
    ``max_steps`` (an int >= H, or None: 8 H; with ``"tile"`` only): the accepted steps a tile may KEEP over the whole
    horizon when a backward follows — slots are counted per tile across the intervals, not per interval.  The kept
    buffers are max_steps x 7 stages x B rows of what the grid kernels keep per stage; per row and slot, with n_g = n_s
    n_u: input gradients 7 (4 n_g + 112) bytes (g(x) and the seven layers' mask words); parameter gradients
    7 (4 n_g + 4 n_s + 28 hid + 112) bytes forward (g(x), the stage inputs, seven layers of activation rows, the words)
    and 7 (4 n_g + 4 n_s + 28 hid) more in the backward; nothing under ``torch.no_grad``, where ``max_steps`` is no
    limit either.  ``max_steps * 7 * B >= 2**31`` is a ``ValueError``.
    ``info`` (a dict or None; with ``"tile"`` only) receives device tensors, without a synchronisation: ``accepted`` and
    ``attempts`` (n_tiles, H) int32 — the steps of every tile in every interval — and ``status`` (n_tiles,) int32: 0 ok,
    1 out of step slots, 2 more than 1000 attempts in an interval (the chained solve's own cap).  A tile that stops
    writes NaN into its rows of ``out`` from that interval on; the forward never synchronises, and the backward — which
    reads ``status`` first, one small copy to the host — raises ``NlbacError`` naming ``max_steps`` and the largest
    count seen.

    ``tile_steps`` (with ``"tile"`` only, and in place of ``max_steps``: giving both is a ``ValueError``) counts the
    slots PER TILE.  ``max_steps`` sizes every tile's slots for the tile that takes the most steps; where the tiles
    differ, most of what it allocates, zero-fills and hands to the weight-gradient launch holds nothing.  A sequence of
    ints or a 1-D integer CPU tensor with one entry per tile (``n_tiles = ceil(B / 32)``; every entry an int >= H; a
    CUDA tensor is a ``ValueError`` — the forward would have to wait for it) gives tile j exactly ``tile_steps[j]``
    slots for the whole horizon.  The kept buffers then hold ``sum(tile_steps)`` PAGES of 7 stages x 32 rows instead of
    ``max_steps * n_tiles`` of them — per page 32 x the per-row-and-slot bytes above: input gradients 224 (4 n_g + 112)
    bytes; parameter gradients 224 (4 n_g + 4 n_s + 28 hid + 112) forward and 224 (4 n_g + 4 n_s + 28 hid) more in
    the backward (a partial last tile still has whole pages) — and the weight-gradient launch walks ``sum(tile_steps)
    * 7 * 32`` rows; ``sum(tile_steps) * 7 * 32 >= 2**31`` is a ``ValueError``.  ``out`` and the input gradients are
    those of a ``max_steps`` call that suffices, bit for bit; the parameter gradients are summed over the rows in
    another order.  A tile that needs more than its own count stops as above (status 1, NaN rows), and the backward's
    ``NlbacError`` names ``tile_steps`` and that tile's count.  The forward still never synchronises.
    ``tile_steps="count"``: the solve counts first — the forward launch runs once with nothing kept (the same kernel
    instance as the kept launch, hence the same steps: no headroom is needed), the tiles' counts of accepted steps come
    to the host, and the kept forward runs with exactly those.  That costs ONE EXTRA FORWARD LAUNCH AND ONE HOST WAIT per
    call; under ``torch.no_grad()`` nothing is kept and nothing is counted.  ``info`` also receives ``slots``: the int32
    CPU tensor of per-tile counts the buffers were sized with (None where nothing was kept and nothing given) — pass it
    back in as ``tile_steps`` on the next call over similar inputs to save the counting pass."""
    T.check_adjoint_chunk("rollout", adjoint, adjoint_chunk, chained=method == "dopri5")
    # (the default call is the call as it was; the step-control arguments go along only where one of them is given)
    tile_args = {} if (step_control == "batch" and max_steps is None and info is None and tile_steps is None) else dict(
        adjoint=adjoint, step_control=step_control, max_steps=max_steps, info=info)
    if tile_steps is not None:
        tile_args["tile_steps"] = tile_steps
    dt, hs = _check(func, x0, controls, dt, method, step_size, **tile_args)
    slots = None if step_control == "batch" else (8 * controls.shape[0] if max_steps is None else max_steps)
    params = tuple(func.parameters())
    mode = T.keep_mode(params, x0, controls)
    func.refresh_device_weights()
    H, plan = controls.shape[0], None
    if tile_steps is not None:
        iv = T.TileSteps(dt, H, None, info, T.tile_steps_arg(tile_steps))
    elif slots is not None:
        iv = T.TileSteps(dt, H, slots, info)
    else:
        iv = T.EqualSteps(dt, H) if hs is None else T.HeldSteps(hs, H, x0.device)
        if adjoint:
            plan = T.AdjointPlan([(dt,) if hs is None else hs] * H, True, adjoint_chunk, hs is not None)
    solve = _RolloutSolve(func, method, iv, float(atol), float(rtol), mode, plan)
    return SolveNode.apply(solve, 2, x0, controls, *params)


def _one_launch_ok(func, method):
    return bool(ONE_LAUNCH and method in ("euler", "rk4") and T.traj_class(func).ok(func))


class _RolloutSolve:
    """One rollout as ``ode_node.SolveNode``'s solve, inputs (x0, controls): direct, with an ``AdjointPlan`` the
    continuous adjoint — what is saved for the backward is then ``out`` (as a saved tensor) and the controls — and with
    ``TileSteps`` dopri5 under tile-local step control (always one launch)."""
    api = "rollout"

    def __init__(self, func, method, iv, atol, rtol, mode, plan=None):
        self.func, self.method, self.iv, self.tol, self.mode, self.plan = func, method, iv, (atol, rtol), mode, plan
        self.with_params, self.saves_out, self.kept = mode == "params", plan is not None, None

    def forward(self, x0, controls):
        func, iv, H = self.func, self.iv, controls.shape[0]
        x0, u = x0.contiguous(), controls.contiguous()
        out = torch.empty(H + 1, x0.shape[0], func.n_s, dtype=torch.float32, device=x0.device)
        first = out[0].copy_(x0)
        one = isinstance(iv, T.TileSteps) or _one_launch_ok(func, self.method)
        # (the one launch reads x0 where the caller's tensor is; the chain's first solver keeps a reference, to out[0])
        args = (x0 if one else first, u, out.narrow(0, 1, H), *self.tol)
        if self.plan is None:
            self.kept = T.solve(func, iv, self.method, self.mode, one, *args)
        else:
            self.kept = T.solve_adjoint(func, iv, self.method, self.mode, one, self.plan, *args)
        return out

    def backward(self, dout, need_in, need_p, out=None):
        return self.kept.backward(dout.contiguous(), need_p, out=out)
