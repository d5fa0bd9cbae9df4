"""What ``rollout`` and ``ode_grid.odeint_grid`` share: a NODE solved over H intervals as one autograd node.

  * the intervals (``EqualSteps``: one ``dt`` and a control per interval, ``rollout``; ``GridSteps``: a step per
    interval and one set of controls, ``odeint_grid``; ``SubGridSteps``: the fine intervals of ``odeint_grid`` under
    ``step_size``, whose output points are interpolated; ``HeldSteps``: the fine intervals of ``rollout`` under
    ``step_size``, a control held over each m of them): the entry points' infix, their step arguments, what the
    controls' gradient looks like, where the outputs and their gradients meet the intervals;
  * what a solve keeps and how its backward becomes gradients, one class per path — ``AffineTraj`` / ``ConcatTraj`` (one
    launch forward, one backward, + the weight-gradient launch over all H * stages * rows) and ``Chain`` (H one-interval
    solves on the existing solvers) — each with ``forward(x0, u, xs)`` and ``backward(dout, need_p, out=None)``;
    ``solve`` picks; beside them dopri5 under tile-local step control, one launch each way over step slots: ``AffineTile`` owns what such
    a solve keeps, the look at its status in front of a backward and its weight gradients; its leaves their own arrays
    and launches — ``AffineTileDopri`` for ``TileSteps`` (``rollout(step_control="tile")``), ``AffineTileDense`` for one
    dense solve per tile read at every point of a time grid (``ode_dense.odeint_dense(step_control="tile")``); every
    class of a form shares ``_kept_acts`` and ``_affine_weight_grads`` / ``_concat_weight_grads``;
  * the same under ``adjoint=True`` (``solve_adjoint``): nothing kept but the outputs the caller holds and the controls —
    ``AdjointPlan`` (per output interval the fine steps of its backward solve, the chunk), ``AffineAdjTraj`` /
    ``ConcatAdjTraj`` (the continuous adjoint over the whole horizon in one ``nlbac_*_adj_traj`` launch per chunk),
    ``Chain(adjoint=True)`` / ``ChainSubAdjoint`` (chained); the same ``backward``, which here needs ``out``.
"""
import ctypes as C
import numbers

import torch

from . import _lib
from ._lib import fptr
from .arena import bwd_weights, io_array, mlp_array, stream_ptr
from .ode_consts import DP_C_ERR, TABLEAU, env_switch
from .ode_node import _reduce
from .odeint import AffineNodeSolver, ConcatNodeSolver


def keep_mode(params, *inputs):
    """What is kept for the backward: activation rows ("params"), ReLU mask words ("inputs") or nothing ("none")."""
    if not torch.is_grad_enabled():
        return "none"
    if any(p.requires_grad for p in params):
        return "params"
    return "inputs" if any(t.requires_grad for t in inputs) else "none"


class _OutputPerInterval:
    """Output k + 1 is the state behind interval k (the chained path's hooks; the one-launch kernels do the same)."""

    @property
    def n_out(self):
        return self.H

    @property
    def launch_H(self):                       # the entry points' H argument (the intervals their controls / outputs count)
        return self.H

    def emit(self, xs, k, x_old, x_new):      # interval k's result into the outputs; returns the next interval's state
        return xs[k].copy_(x_new)

    def grad_in(self, dout, k, carry):        # dL/dx_{k+1} = dout[k+1] + what interval k+1 sends back
        return dout[k + 1] if carry is None else (dout[k + 1] + carry)

    def grad_carry(self, dout, k, dy0):       # what interval k sends back to interval k-1
        return dy0.clone()

    def sum_copied(self, d):                  # d (n_out, n, n_c): the gradients of the columns copied to every output
        return d.sum(0)


class EqualSteps(_OutputPerInterval):
    """H intervals of ``dt`` with a control per interval: controls (H, n, n_c), their gradient stacked per interval."""
    api, infix, solvers_key = "rollout", "traj", "_rollout_solvers"

    def __init__(self, dt, H):
        self.dt, self.H = dt, H

    def step_args(self):
        return (self.dt,)

    def step(self, k):
        return self.dt

    def control(self, u, k):
        return u[k]

    def du_shape(self, n, nc):
        return (self.H, n, nc)

    def add_du(self, acc, k, du):
        if acc is None:
            acc = torch.empty(self.H, *du.shape, dtype=torch.float32, device=du.device)
        acc[k].copy_(du)
        return acc

    def slabs(self, arena, sv):      # (dopri5: the interval's accepted steps share the slabs)
        n_steps = max(1, len(sv.ctx.get("steps") or [None]))
        return max(1, arena.n_slabs // n_steps)


class GridSteps(_OutputPerInterval):
    """The intervals of a time grid, steps ``hs``, with one set of controls (n, n_c) for all of them, whose gradient is
    summed over the intervals."""
    api, infix, solvers_key = "odeint_grid", "grid", "_odeint_grid_solvers"

    def __init__(self, hs, device):
        self.hs, self.H, self.device, self.arrays = hs, len(hs), device, None

    def step_args(self):
        if self.arrays is None:      # the steps twice: on the device for the kernels, in host memory for the launcher's checks
            self.arrays = (torch.tensor(self.hs, dtype=torch.float32, device=self.device), fptr(*self.hs))
        return (self.arrays[0].data_ptr(), self.arrays[1])

    def step(self, k):
        return self.hs[k]

    def control(self, u, k):
        return u

    def du_shape(self, n, nc):
        return (n, nc)

    def add_du(self, acc, k, du):      # k = H-1 .. 0: the order of the one-launch kernels' sum
        return du.clone() if acc is None else acc + du

    def slabs(self, arena, sv):
        return arena.n_slabs


class SubGridSteps(GridSteps):
    """The N fine intervals of a time grid solved under ``step_size`` (``ode_grid._sub_grid``): steps ``hs``, and the
    T - 1 output points 1 .. T-1 read off them — interval i holds the outputs ofs[i] <= j < ofs[i+1], output j is
    y_i + theta[j-1] (y_{i+1} - y_i), the fine state itself at theta 1 / 0.  The one-launch kernels
    (``nlbac_*_rk_subgrid_*``) take ``ofs`` / ``theta`` beside the steps; the chained path interpolates, and injects the
    output gradients between the fine intervals, with the torch ops below — in the kernels' order."""
    infix, solvers_key = "subgrid", "_odeint_subgrid_solvers"

    def __init__(self, hs, ofs, theta, device):
        GridSteps.__init__(self, hs, device)
        self.ofs, self.theta = ofs, theta

    @property
    def n_out(self):
        return len(self.theta)

    def step_args(self):
        if self.arrays is None:      # steps, offsets and weights twice each: device for the kernels, host for the launcher
            dev = lambda v, dt: torch.tensor(v, dtype=dt, device=self.device)
            self.arrays = (dev(self.hs, torch.float32), fptr(*self.hs), dev(self.ofs, torch.int32),
                           (C.c_int * len(self.ofs))(*self.ofs), dev(self.theta, torch.float32), fptr(*self.theta))
        a = self.arrays
        return (a[0].data_ptr(), a[1], a[2].data_ptr(), a[3], a[4].data_ptr(), a[5], len(self.theta) + 1)

    def emit(self, xs, k, x_old, x_new):
        x_new = x_new.clone()
        for j in range(self.ofs[k], self.ofs[k + 1]):
            th = self.theta[j - 1]
            xs[j - 1].copy_(x_new if th == 1.0 else (x_old if th == 0.0 else x_old + th * (x_new - x_old)))
        return x_new

    def grad_in(self, dout, k, carry):        # sum_j theta_j dout[j] (j ascending), then what interval k+1 sends back
        d = torch.zeros_like(dout[0])
        for j in range(self.ofs[k], self.ofs[k + 1]):
            d = d + self.theta[j - 1] * dout[j]
        return d if carry is None else d + carry

    def grad_carry(self, dout, k, dy0):       # the outputs' share of the interval's own initial state
        dy0 = dy0.clone()
        for j in range(self.ofs[k], self.ofs[k + 1]):
            if self.theta[j - 1] < 1.0:
                dy0 = dy0 + C.c_float(1.0 - self.theta[j - 1]).value * dout[j]
        return dy0

    def sum_copied(self, d):
        # per fine interval first (j ascending), then over the fine intervals as GridSteps sums over its intervals: with
        # every weight 1 the bits of the solve on the fine grid itself with zero gradients at the unused points
        per = torch.zeros(self.H, *d.shape[1:], dtype=d.dtype, device=d.device)
        for k in range(self.H):
            for j in range(self.ofs[k], self.ofs[k + 1]):
                per[k] += d[j - 1]
        return per.sum(0)


class HeldSteps(_OutputPerInterval):
    """The N = H m fine intervals of a rollout solved under ``step_size``: every control interval is cut into the same m
    fine steps ``hs`` (``ode_grid._sub_grid`` over [0, dt]), its control held through them — fine interval i = k m + r runs
    under controls[k] with step hs[r].  One output per control interval (the fine-grid end point, weight 1: nothing is
    interpolated), the controls' gradient summed inside a control interval and stacked per control interval.  The
    one-launch kernels (``nlbac_*_rk_hold_*``) take ``m`` beside the steps; the chained path does the same with the torch
    ops below — in the kernels' order."""
    api, infix, solvers_key = "rollout", "hold", "_rollout_hold_solvers"

    def __init__(self, hs, H, device):
        self.hs, self.m, self.n_ctl, self.H, self.device, self.arrays = hs, len(hs), H, H * len(hs), device, None

    @property
    def n_out(self):
        return self.n_ctl

    @property
    def launch_H(self):
        return self.n_ctl

    def step_args(self):
        if self.arrays is None:      # the steps twice: on the device for the kernels, in host memory for the launcher's checks
            self.arrays = (torch.tensor(self.hs, dtype=torch.float32, device=self.device), fptr(*self.hs))
        return (self.arrays[0].data_ptr(), self.arrays[1], self.m)

    def step(self, i):
        return self.hs[i % self.m]

    def control(self, u, i):
        return u[i // self.m]

    def du_shape(self, n, nc):
        return (self.n_ctl, n, nc)

    def emit(self, xs, i, x_old, x_new):      # out[k] behind the control interval's last fine step only
        k, r = divmod(i, self.m)
        return xs[k].copy_(x_new) if r == self.m - 1 else x_new.clone()

    def grad_in(self, dout, i, carry):        # dout[k+1] comes in behind r = m-1; elsewhere d = 0 + what interval i+1 sends back
        k, r = divmod(i, self.m)
        if r == self.m - 1:
            return dout[k + 1] if carry is None else (dout[k + 1] + carry)
        return torch.zeros_like(carry) + carry

    def add_du(self, acc, i, du):             # i = N-1 .. 0: total = du_{m-1}; total = total + du_r, per control interval
        k, r = divmod(i, self.m)
        if acc is None:
            acc = torch.empty(self.n_ctl, *du.shape, dtype=torch.float32, device=du.device)
        acc[k].copy_(du if r == self.m - 1 else acc[k] + du)
        return acc

    def slabs(self, arena, sv):
        return arena.n_slabs


def _tableau(method):
    """(S, beta, c_out) as the launchers take them: a stage per row of the table and the one in place, the table flat
    [S][S] with its row i as row i + 1, and the solution weights (None where the method has none: dopri5)."""
    tab = TABLEAU[method]
    S = len(tab["beta"]) + 1
    beta = [0.0] * (S * S)
    for i, r in enumerate(tab["beta"]):
        for j, v in enumerate(r):
            beta[(i + 1) * S + j] = v
    return S, fptr(*beta), fptr(*tab["c_sol"]) if tab["c_sol"] is not None else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _acts_bits(mode):
    """The entry points' ``acts_bits`` of keep mode ``mode`` — which also picks the kernel instance of a launch that
    keeps nothing."""
    words = mode == "inputs" or (mode == "params" and env_switch("fit_words"))
    return 0 if mode == "none" else (1 if mode == "inputs" else (2 if words else 0))


def _kept_acts(f, g, rows, mode, alloc):
    """What the control-affine form keeps of the hidden layers over ``rows`` stage rows (stages * n), from ``alloc``:
    (acts_bits, the two nets' buffers, their layer strides)."""
    bits = _acts_bits(mode)
    words = bits != 0
    acts, ls = [None, None], [0, 0]
    if mode != "none":
        for i, net in enumerate((f, g)):
            nw = net.n_layers - 1
            if mode == "inputs":                       # words in place of the rows
                acts[i], ls[i] = alloc(nw * rows * 4, dtype=torch.int32), rows * 4
            else:                                      # rows [layer][rows][hid], then (bits 2) words [layer][rows][4]
                acts[i] = alloc(nw * rows * (net.hid + (4 if words else 0)))
                ls[i] = rows * net.hid
    return bits, acts, ls


def _affine_weight_grads(f, g, x0, x0_ld, dys, acts, acts_ls, dzs, rows, dev):
    """The control-affine form's weight gradients: ``rows`` stage rows as ONE batch through the weight-gradient launch,
    then the slabs' sum.  ``x0`` / ``x0_ld``: where layer 0's input rows (n_s columns) lie and their leading dimension;
    per net (f, g) the output gradients ``dys`` = (dK, dG), the ``acts`` pointers with their layer strides, ``dzs``."""
    arena = f.arena
    io = io_array(2)
    for i in range(2):
        io[i].x0, io[i].x0_dim, io[i].x0_ld = x0, dys[0].shape[-1], x0_ld
        io[i].dy, io[i].dy_ld = dys[i].data_ptr(), dys[i].shape[-1]
        io[i].acts, io[i].acts_ls = acts[i], acts_ls[i]
        io[i].dz = dzs[i].data_ptr()
        io[i].grad = arena.grad.data_ptr()
    bwd_weights(mlp_array([f.desc, g.desc]), io, 2, rows, arena.n_slabs, arena.n, dev)
    return _reduce(arena, arena.n_slabs)


def _concat_weight_grads(net, xin, in_dim, dy, acts, acts_ls, dz, rows, dev):
    """The single-net form's weight gradients, as ``_affine_weight_grads``: layer 0's input is the kept row at ``xin``
    (``in_dim`` columns)."""
    arena = net.arena
    io = io_array(1)
    io[0].x0, io[0].x0_dim, io[0].x0_ld = xin, in_dim, in_dim
    io[0].dy, io[0].dy_ld = dy.data_ptr(), dy.shape[-1]
    io[0].acts, io[0].acts_ls = acts, acts_ls
    io[0].dz = dz.data_ptr()
    io[0].grad = arena.grad.data_ptr()
    bwd_weights(mlp_array([net.desc]), io, 1, rows, arena.n_slabs, arena.n, dev)
    return _reduce(arena, arena.n_slabs)


class AffineTraj:
    """Device buffers of one one-launch solve of the control-affine NODE: step-major [k][stage][row] over H * S stages."""
    Solver = AffineNodeSolver
    dx0_total = True      # ``backward`` takes all of dout and returns dx0 with dout[0] inside (``ode_node.PackedSolve.grad_y0``)

    @staticmethod
    def ok(func):
        f, g = func.device_handles()
        return _lib.load().nlbac_node_rk_traj_ok(C.byref(f.desc), C.byref(g.desc)) == 1

    def __init__(self, func, n, iv, method, mode, device):
        f, g = func.device_handles()
        self.f, self.g, self.iv = f, g, iv
        self.ns, self.nu = func.n_s, func.n_u
        self.S, self.beta, self.c_out = _tableau(method)
        self.n, self.H = n, iv.H
        HS = iv.H * self.S
        z = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=device)
        self.K, self.Y, self.G = z(HS, n, self.ns), z(HS, n, self.ns), z(HS, n, self.ns * self.nu)
        self.bits, self.acts, self.ls = _kept_acts(f, g, HS * n, mode, z)

    def forward(self, x0, u, xs):
        self.u = u
        _lib.call("nlbac_node_rk_%s_fwd" % self.iv.infix, C.byref(self.f.desc), C.byref(self.g.desc), x0.data_ptr(),
                  u.data_ptr(), self.n, self.iv.launch_H, self.S, self.beta, self.c_out, *self.iv.step_args(),
                  xs.data_ptr(), self.K.data_ptr(), self.Y.data_ptr(), self.G.data_ptr(), _ptr(self.acts[0]), self.ls[0],
                  _ptr(self.acts[1]), self.ls[1], self.bits, stream_ptr())

    def backward(self, dout, need_p, out=None):
        n, H, S, HS = self.n, self.iv.launch_H, self.S, self.H * self.S      # (H: the launch's; HS: the stages kept)
        dev = dout.device
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dx0, du = z(n, self.ns), z(*self.iv.du_shape(n, self.nu))
        dK = dG = dz_f = dz_g = None
        if need_p:
            dK, dG = z(HS, n, self.ns), z(HS, n, self.ns * self.nu)
            dz_f, dz_g = z(self.f.n_layers - 1, HS * n, self.f.hid), z(self.g.n_layers - 1, HS * n, self.g.hid)
        _lib.call("nlbac_node_rk_%s_bwd" % self.iv.infix, C.byref(self.f.desc), C.byref(self.g.desc), self.u.data_ptr(),
                  n, H, S, self.beta, self.c_out, *self.iv.step_args(), self.G.data_ptr(), _ptr(self.acts[0]),
                  self.ls[0], _ptr(self.acts[1]), self.ls[1], self.bits, dout.data_ptr(), dx0.data_ptr(), du.data_ptr(),
                  _ptr(dK), _ptr(dG), _ptr(dz_f), _ptr(dz_g), stream_ptr())
        if not need_p:
            return dx0, du, None
        # every stage of every interval as ONE batch of H * S * n rows through the weight-gradient launch
        return dx0, du, _affine_weight_grads(self.f, self.g, self.Y.data_ptr(), self.ns, (dK, dG),
                                             [_ptr(a) for a in self.acts], self.ls, (dz_f, dz_g), HS * n, dev)


class ConcatTraj:
    """Device buffers of one one-launch solve of the single-net NODE, step-major [k][stage][row] over H * S stages:
    nothing without gradients, the three layers' mask words for input gradients, activation rows and the stage-input
    rows layer 0 saw ([Y_st | c_k], normalised when the net is) for parameter gradients."""
    Solver = ConcatNodeSolver
    dx0_total = True

    @staticmethod
    def ok(func):
        return _lib.load().nlbac_concat_rk_traj_ok(C.byref(func.device_handles()[0].desc)) == 1

    def __init__(self, func, n, iv, method, mode, device):
        self.net, self.iv = func.device_handles()[0], iv
        self.ns, self.nc = func.n_s, func.n_carry
        self.S, self.beta, self.c_out = _tableau(method)
        self.n, self.H = n, iv.H
        self.norm = func.norm_device() if getattr(func, "normalized", False) else None
        HS, nw = iv.H * self.S, self.net.n_layers - 1
        self.bits = 1 if mode == "inputs" else 0
        self.acts, self.ls, self.Xin = None, 0, None
        if mode == "inputs":
            self.acts, self.ls = torch.empty(nw * HS * n * 4, dtype=torch.int32, device=device), HS * n * 4
        elif mode == "params":
            self.acts = torch.empty(nw, HS * n, self.net.hid, dtype=torch.float32, device=device)
            self.ls = HS * n * self.net.hid
            self.Xin = torch.empty(HS * n, self.net.in_dim, dtype=torch.float32, device=device)

    def forward(self, x0, u, xs):
        _lib.call("nlbac_concat_rk_%s_fwd" % self.iv.infix, C.byref(self.net.desc), x0.data_ptr(), u.data_ptr(), self.n,
                  self.iv.launch_H, self.S, self.beta, self.c_out, *self.iv.step_args(), xs.data_ptr(), _ptr(self.Xin),
                  _ptr(self.acts), self.ls, self.bits, _ptr(self.norm), stream_ptr())

    def backward(self, dout, need_p, out=None):
        n, H, S, HS = self.n, self.iv.launch_H, self.S, self.H * self.S      # (H: the launch's; HS: the stages kept)
        dev = dout.device
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dx0, du = z(n, self.ns), z(*self.iv.du_shape(n, self.nc))
        dK = dz = None
        if need_p:
            dK, dz = z(HS * n, self.ns), z(self.net.n_layers - 1, HS * n, self.net.hid)
        _lib.call("nlbac_concat_rk_%s_bwd" % self.iv.infix, C.byref(self.net.desc), n, H, S, self.beta, self.c_out,
                  *self.iv.step_args(), self.acts.data_ptr(), self.ls, self.bits, _ptr(self.norm), dout.data_ptr(),
                  dx0.data_ptr(), du.data_ptr(), _ptr(dK), _ptr(dz), stream_ptr())
        if not need_p:
            return dx0, du, None
        # every stage of every interval as ONE batch of H * S * n rows: layer 0's input is the kept Xin row
        return dx0, du, _concat_weight_grads(self.net, self.Xin.data_ptr(), self.net.in_dim, dK, self.acts.data_ptr(),
                                             self.ls, dz, HS * n, dev)


def tile_steps_arg(tile_steps):
    """``tile_steps`` as the solve classes take it: None, ``"count"`` or a 1-D int32 CPU tensor (``check_tile_steps`` has
    checked it)."""
    if tile_steps is None or isinstance(tile_steps, str):
        return tile_steps
    if isinstance(tile_steps, torch.Tensor):
        return tile_steps.to(torch.int32)
    return torch.tensor([int(v) for v in tile_steps], dtype=torch.int32)


_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def check_tile_steps(api, tile_steps, n, least, why):
    """The checks of a ``tile_steps`` that is not None, for ``n`` rows — nothing here touches a device: ``"count"``, or
    one int >= ``least`` per 32-row tile (``why``: what the least stands for) as a sequence or a 1-D integer CPU tensor,
    ``sum * 7 * 32`` below 2^31.  (A tensor is checked as a whole: no Python loop over the tiles of a large batch.)"""
    if isinstance(tile_steps, str):
        if tile_steps != "count":
            raise ValueError("%s: tile_steps is None, 'count' or one int per tile; got %r" % (api, tile_steps))
        return
    if isinstance(tile_steps, torch.Tensor):
        if tile_steps.device.type != "cpu":
            raise ValueError("%s: tile_steps must be a CPU tensor (pass tile_steps.cpu(): the forward does not "
                             "synchronise behind the caller's back); got one on %s" % (api, tile_steps.device))
        if tile_steps.dim() != 1 or tile_steps.dtype not in _INT_DTYPES:
            raise ValueError("%s: a tile_steps tensor is 1-D and of an integer dtype; got %s of %s"
                             % (api, tuple(tile_steps.shape), tile_steps.dtype))
        count = tile_steps.numel()
        low, total = (int(tile_steps.min()), int(tile_steps.sum(dtype=torch.int64))) if count else (least, 0)
    else:
        try:
            vals = list(tile_steps)
        except TypeError:
            raise ValueError("%s: tile_steps is None, 'count' or one int per tile (a sequence or a 1-D integer CPU "
                             "tensor); got %s" % (api, type(tile_steps).__name__)) from None
        if set(map(type, vals)) - {int}:      # (anything but plain ints: look at each)
            for v in vals:
                if isinstance(v, torch.Tensor):
                    raise ValueError("%s: the entries of tile_steps are Python ints (a tensor goes in whole, as a 1-D "
                                     "integer CPU tensor); got a sequence of tensors" % api)
                if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                    raise ValueError("%s: every entry of tile_steps must be an int; got %r" % (api, v))
        count = len(vals)
        low, total = (min(vals), sum(vals)) if count else (least, 0)
    tiles = (n + _lib.MLP_TILE - 1) // _lib.MLP_TILE
    if count != tiles:
        raise ValueError("%s: tile_steps has one entry per 32-row tile, %d for %d rows; got %d" % (api, tiles, n, count))
    if low < least:
        raise ValueError("%s: every entry of tile_steps must be >= %d (%s); got %d" % (api, least, why, low))
    if total * 7 * _lib.MLP_TILE >= 2 ** 31:
        raise ValueError("%s: sum(tile_steps) * 7 stages * 32 rows is 2^31 or more (the launch's limit: %d * 7 * 32); use "
                         "fewer slots or fewer rows" % (api, total))


class TileSteps(EqualSteps):
    """``EqualSteps`` solved by dopri5 under tile-local step control (``rollout(step_control="tile")``): every 32-row tile
    an adaptive solve of its own, ``max_steps`` step slots per tile for the whole horizon when a backward follows — or,
    with ``tile_steps`` (``tile_steps_arg``'s: ``"count"`` or a tensor, ``max_steps`` then None), a count of its own per
    tile; ``info`` (a dict or None) receives the solve's device tensors."""

    def __init__(self, dt, H, max_steps, info=None, tile_steps=None):
        EqualSteps.__init__(self, dt, H)
        self.max_steps, self.info, self.tile_steps = max_steps, info, tile_steps


class AffineTile:
    """What a dopri5 solve of the control-affine NODE under tile-local step control keeps, whichever way its outputs are
    read (``AffineTileDopri``, ``AffineTileDense``): the nets, tolerances and dopri5's table, every tile's counts and
    status, and — when a backward follows — the kept buffers, slot-major [slot][stage][row] over max_steps * 7 stages, a
    slot per accepted step of a tile: ``AffineTraj``'s layout with the slot in place of the interval; zero-filled, so
    that a stage nobody evaluated (a slot a tile did not use, stage 0 of a step that took it from the step before) adds
    nothing to the weight gradients.  A leaf has ``api`` and ``words`` (what differs in the stopped-tile message),
    ``least`` (the slots a tile needs at least), ``du_shape``, ``_nacc()``, the arrays that say where its outputs lie in
    the slots, and its launches ``_fwd`` / ``_bwd``.

    With ``tile_steps`` (``tile_steps_arg``'s) the slots are counted per tile and the kept buffers are PAGED: tile j owns
    ``slots[j]`` pages of 7 stages x 32 rows, the buffers hold ``pages = sum(slots)`` of them — [page][stage][32 rows],
    the layout above with 32 in place of n and the page in place of the slot — and ``page0``, the exclusive prefix sum,
    goes to the device once; the launches are the ``*_paged_*`` entry points.  ``"count"``: the forward first runs the
    same entry with nothing kept, brings the tiles' counts of accepted steps to the host (the one wait of such a
    forward) and sizes the buffers by exactly those."""
    S = 7

    @staticmethod
    def shapes_ok(func):
        """What the library's ``nlbac_node_dopri_tile_ok`` asks of the nets, from their shapes alone (no device, no
        library: ``rollout._check`` runs before either)."""
        if not func.affine:
            return False
        lin = lambda net: [m for m in net.modules() if isinstance(m, torch.nn.Linear)]
        f, g = lin(func.f_net), lin(func.g_net)
        hid = f[0].out_features
        return (len(f) == 5 and len(g) == 4 and hid in (64, 100, 128) and g[0].out_features == hid and
                1 <= func.n_s <= 8 and 1 <= func.n_u <= 4 and ((func.n_s + 3) // 4) * func.n_u <= 4)

    @staticmethod
    def ok(func):
        if not func.affine:
            return False
        f, g = func.device_handles()
        return _lib.load().nlbac_node_dopri_tile_ok(C.byref(f.desc), C.byref(g.desc)) == 1

    def __init__(self, func, n, counts, max_steps, info, mode, atol, rtol, device, tile_steps=None):
        """``counts``: the shape of a tile's ``accepted`` / ``attempts`` (a count per interval; one for a dense solve)."""
        if not self.ok(func):
            raise NotImplementedError("%s: step_control='tile' needs nets the register-resident kernels serve "
                                      "(nlbac_node_dopri_tile_ok); there is no chained fallback" % self.api)
        f, g = func.device_handles()
        self.f, self.g, self.info, self.mode, self.tol = f, g, info, mode, (rtol, atol)
        self.ns, self.nu, self.n = func.n_s, func.n_u, n
        self.beta, self.c_err = _tableau("dopri5")[1], fptr(*DP_C_ERR)
        self.tiles = (n + _lib.MLP_TILE - 1) // _lib.MLP_TILE
        self.device, self.counts, self.paged = device, counts, tile_steps is not None
        self._counters()
        self.M = self.pages = 0      # (the slots every tile has; paged: the pages of all tiles)
        self.G = self.Y = self.hslots = self.slots = self.page0 = None
        self.bits, self.acts, self.ls = _acts_bits(mode), [None, None], [0, 0]
        counting = isinstance(tile_steps, str)      # ("count": the buffers wait for the forward's first pass)
        if self.paged and not counting:
            self.slots = tile_steps
        if mode != "none" and not counting:
            self._keep(tile_steps if self.paged else max_steps)

    def _counters(self):
        z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.device)
        self.accepted, self.attempts, self.status = z(self.tiles, *self.counts), z(self.tiles, *self.counts), z(self.tiles)

    def _keep(self, slots):
        """The kept buffers (zero-filled): ``slots`` an int — that many slots for every tile, [slot][stage][n rows] — or
        an int32 CPU tensor, one count per tile: paged."""
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        if self.paged:
            self.slots = slots
            page0 = torch.zeros(self.tiles + 1, dtype=torch.int32)
            torch.cumsum(slots, 0, dtype=torch.int32, out=page0[1:])
            self.pages = int(page0[-1])
            self.page0 = page0.to(self.device)
            stages, rows, hs = self.pages * self.S, _lib.MLP_TILE, (self.pages,)
        else:
            self.M = slots
            stages, rows, hs = self.M * self.S, self.n, (self.tiles, self.M)
        self.G = z(stages, rows, self.ns * self.nu)
        self.Y = z(stages, rows, self.ns) if self.mode == "params" else None
        self.hslots = z(*hs, dtype=torch.float64)
        self._interval_arrays(z)
        self.bits, self.acts, self.ls = _kept_acts(self.f, self.g, stages * rows, self.mode, z)

    def _interval_arrays(self, z):
        """A leaf's kept arrays that come between ``hslots`` and the activations in the order of allocation."""

    def _slot_args(self):
        """What the entry points take for the slots: ``max_slots``, or (paged) ``page0`` and the pages."""
        return (_ptr(self.page0), self.pages) if self.paged else (self.M,)

    def forward(self, x0, u, xs):
        self.u = u
        if self.paged and self.G is None and self.mode != "none":
            # tile_steps="count": the launch as it will be kept (acts_bits picks the same kernel instance, so the steps
            # are the same), nothing kept; the tiles' counts come to the host, and the buffers hold exactly those
            self._fwd(x0, u, xs, *self.tol)
            seen = self._nacc().cpu().clamp_(min=self.least)      # (a tile that stopped at the attempt cap stops again)
            self._counters()
            self._keep(seen)
        self._fwd(x0, u, xs, *self.tol)
        if self.info is not None:
            self.info.update(accepted=self.accepted, attempts=self.attempts, status=self.status)
            if self.paged:
                self.info.update(slots=self.slots)

    def backward(self, dout, need_p, out=None):
        """``dout``: the outputs' gradients as the leaf's launch takes them.  Returns (dx0: the first step's dy0, the
        controls' gradient, the flat parameter gradient or None)."""
        dev = dout.device
        used = self._look()
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dx0, du = z(self.n, self.ns), z(*self.du_shape)
        rows = self._weight_rows(dev) if need_p else (None, None, None, None)
        self._bwd(dout, dx0, du, *[_ptr(r) for r in rows])
        return dx0, du, self._weight_grads(*rows, used, dev) if need_p else None

    def _look(self):
        """The one look at the solve, long after its launch has finished: every tile's status and count of accepted steps
        (the leaf's ``_nacc()``) come to the host.  Returns the largest count, the slots in use; raises if a tile stopped
        (paged: a tile's count is held against its own slots)."""
        seen = torch.stack((self.status, self._nacc())).cpu()
        used = int(seen[1].max())
        bad = seen[0].nonzero().flatten().tolist()
        if bad:
            why = {1: "ran out of step slots", 2: "took more than 1000 attempts" + self.words[0]}
            if self.paged:
                j = bad[0]
                raise _lib.NlbacError(
                    "%s(step_control='tile'): tile %d %s (status %d; %d of %d tiles stopped), so the solve has no "
                    "backward: tile_steps[%d] = %d slots, and the tile had kept %d accepted steps when it stopped — give "
                    "that tile more (info['accepted'] of a max_steps run has the counts), or pass tile_steps='count'"
                    % (self.api, j, why.get(int(seen[0][j]), "stopped"), int(seen[0][j]), len(bad), self.tiles, j,
                       int(self.slots[j]), int(seen[1][j])))
            raise _lib.NlbacError(
                "%s(step_control='tile'): tile %d %s (status %d; %d of %d tiles stopped), so the solve has no "
                "backward: max_steps = %d slots per tile, the largest count of accepted steps a tile had kept when it "
                "stopped or finished is %d — raise max_steps (its default is %s)"
                % (self.api, bad[0], why.get(int(seen[0][bad[0]]), "stopped"), int(seen[0][bad[0]]), len(bad), self.tiles,
                   self.M, used, self.words[1]))
        return used

    def _weight_rows(self, dev):
        """dK, dG, dz_f, dz_g per (slot, stage, row) for the weight gradients (zero-filled; paged: per (page, stage, row))."""
        n, MS = (_lib.MLP_TILE, self.pages * self.S) if self.paged else (self.n, self.M * self.S)
        zero = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        return (zero(MS, n, self.ns), zero(MS, n, self.ns * self.nu), zero(self.f.n_layers - 1, MS * n, self.f.hid),
                zero(self.g.n_layers - 1, MS * n, self.g.hid))

    def _weight_grads(self, dK, dG, dz_f, dz_g, used, dev):
        """Every stage of the USED slots as one batch through the weight-gradient launch: the slots are the leading
        index, so the first used * 7 * n rows of every buffer hold them (the layers' stride stays that of all slots).
        Paged: all pages * 7 * 32 rows — with exact counts every page is a step somebody took."""
        rows = self.pages * self.S * _lib.MLP_TILE if self.paged else used * self.S * self.n
        return _affine_weight_grads(self.f, self.g, self.Y.data_ptr(), self.ns, (dK, dG), [_ptr(a) for a in self.acts],
                                    self.ls, (dz_f, dz_g), rows, dev)


class AffineTileDopri(AffineTile):
    """``AffineTile`` of a rollout (``TileSteps``): one ``nlbac_node_dopri_tile_fwd`` launch for the whole horizon, one
    ``nlbac_node_dopri_tile_bwd`` for its backward (+ the weight-gradient launch over the used slots).  Counts per tile
    and interval; per tile and interval its first slot and the abscissa of its output in its last step (``iv_first`` /
    ``iv_x``)."""
    api, words = "rollout", (" in one interval", "8 H")

    def __init__(self, func, n, iv, mode, atol, rtol, device):
        self.iv, self.H, self.du_shape, self.least = iv, iv.H, (iv.H, n, func.n_u), iv.H
        self.iv_first = self.iv_x = None
        AffineTile.__init__(self, func, n, (iv.H,), iv.max_steps, iv.info, mode, atol, rtol, device, iv.tile_steps)

    def _interval_arrays(self, z):
        self.iv_first, self.iv_x = z(self.tiles, self.H, dtype=torch.int32), z(self.tiles, self.H)

    def _nacc(self):
        return self.accepted.sum(1, dtype=torch.int32)

    def _fwd(self, x0, u, xs, rtol, atol):
        _lib.call("nlbac_node_dopri_tile_paged_fwd" if self.paged else "nlbac_node_dopri_tile_fwd", C.byref(self.f.desc),
                  C.byref(self.g.desc), x0.data_ptr(), u.data_ptr(), self.n, self.H, self.beta, self.c_err, self.iv.dt,
                  rtol, atol, xs.data_ptr(), *self._slot_args(), _ptr(self.Y),
                  _ptr(self.G), _ptr(self.acts[0]), self.ls[0], _ptr(self.acts[1]), self.ls[1], self.bits,
                  _ptr(self.hslots), _ptr(self.iv_first), _ptr(self.iv_x), self.accepted.data_ptr(),
                  self.attempts.data_ptr(), self.status.data_ptr(), stream_ptr())

    def _bwd(self, dout, dx0, du, dK, dG, dz_f, dz_g):
        _lib.call("nlbac_node_dopri_tile_paged_bwd" if self.paged else "nlbac_node_dopri_tile_bwd", C.byref(self.f.desc),
                  C.byref(self.g.desc), self.u.data_ptr(), self.n, self.H, self.beta, *self._slot_args(),
                  self.hslots.data_ptr(), self.iv_first.data_ptr(), self.accepted.data_ptr(),
                  self.iv_x.data_ptr(), self.G.data_ptr(), _ptr(self.acts[0]), self.ls[0], _ptr(self.acts[1]), self.ls[1],
                  self.bits, dout.data_ptr(), dx0.data_ptr(), du.data_ptr(), dK, dG, dz_f, dz_g, stream_ptr())


class AffineTileDense(AffineTile):
    """``AffineTile`` of one DENSE solve (``odeint_dense(step_control="tile")``): every 32-row tile runs one adaptive
    solve over ``[0, taus[-1]]`` and writes its interpolant at every output time behind the accepted steps — one
    ``nlbac_node_dopri_tile_dense_fwd`` launch, one ``nlbac_node_dopri_tile_dense_bwd`` for its backward (+ the
    weight-gradient launch over the used slots).  One count per tile; per tile and output the slot that emitted it and
    its abscissa (``ov_slot`` / ``ov_x``).  ``backward`` takes dxs (T - 1, n, n_s): d loss / d out[1:] on the state
    columns."""
    api, words, least = "odeint_dense", ("", "32"), 1
    dx0_total = False     # (``backward`` takes dout[1:]: dout[0] is added behind it)

    def __init__(self, func, n, taus, max_steps, info, mode, atol, rtol, device, tile_steps=None):
        AffineTile.__init__(self, func, n, (), max_steps, info, mode, atol, rtol, device, tile_steps)
        self.n_out, self.t_end, self.du_shape = len(taus), taus[-1], (n, func.n_u)
        self.tau = torch.tensor(taus, dtype=torch.float64, device=device)
        self.ov_slot = self.ov_x = None
        if mode != "none":
            self.ov_slot = torch.zeros(self.tiles, self.n_out, dtype=torch.int32, device=device)
            self.ov_x = torch.zeros(self.tiles, self.n_out, dtype=torch.float32, device=device)

    def _nacc(self):
        return self.accepted

    def _fwd(self, x0, u, xs, rtol, atol):
        _lib.call("nlbac_node_dopri_tile_dense_paged_fwd" if self.paged else "nlbac_node_dopri_tile_dense_fwd",
                  C.byref(self.f.desc), C.byref(self.g.desc), x0.data_ptr(),
                  u.data_ptr(), self.n, self.beta, self.c_err, self.tau.data_ptr(), self.n_out, self.t_end, rtol, atol,
                  xs.data_ptr(), *self._slot_args(), _ptr(self.Y), _ptr(self.G), _ptr(self.acts[0]), self.ls[0], _ptr(self.acts[1]),
                  self.ls[1], self.bits, _ptr(self.hslots), _ptr(self.ov_slot), _ptr(self.ov_x),
                  self.accepted.data_ptr(), self.attempts.data_ptr(), self.status.data_ptr(), stream_ptr())

    def _bwd(self, dxs, dx0, du, dK, dG, dz_f, dz_g):
        _lib.call("nlbac_node_dopri_tile_dense_paged_bwd" if self.paged else "nlbac_node_dopri_tile_dense_bwd",
                  C.byref(self.f.desc), C.byref(self.g.desc), self.u.data_ptr(),
                  self.n, self.beta, self.n_out, *self._slot_args(), self.hslots.data_ptr(), self.ov_slot.data_ptr(),
                  self.ov_x.data_ptr(), self.accepted.data_ptr(), self.G.data_ptr(), _ptr(self.acts[0]), self.ls[0],
                  _ptr(self.acts[1]), self.ls[1], self.bits, dxs.data_ptr(), dx0.data_ptr(), du.data_ptr(), dK, dG, dz_f,
                  dz_g, stream_ptr())


def traj_class(func):
    """The one-launch path of ``func``'s NODE form (the one place that asks which form it is)."""
    return AffineTraj if func.affine else ConcatTraj


class Chain:
    """The chained path: H one-interval solves on the existing solvers, cached on the model under the intervals'
    ``solvers_key`` (apart from ``odeint``'s and any agent task's): one solver per interval when a backward follows (each
    keeps its interval's state), one for all intervals otherwise."""
    dx0_total = True

    def __init__(self, func, n, iv, method, mode, atol, rtol, adjoint=False):
        # (adjoint: solvers of their own whose backward is the continuous adjoint of their interval — the chain of
        #  one-interval ``odeint_adjoint`` calls; each keeps its interval's end state and controls, nothing else)
        self.func, self.n, self.iv, self.method, self.mode, self.tol = func, n, iv, method, mode, (atol, rtol)
        lst = func.__dict__.setdefault(iv.solvers_key + ("_adj" if adjoint else ""), {}).setdefault(mode, [])
        for _ in range((1 if mode == "none" else iv.H) - len(lst)):
            sv = traj_class(func).Solver(func, func.device_handles()[0].arena.device)
            sv.keep_acts = adjoint or mode != "inputs"      # (no grad: the same kernels as odeint's solver; nothing is read back)
            sv.adjoint = bool(adjoint)
            lst.append(sv)
        self.svs = lst[:iv.H]

    def forward(self, x0, u, xs):
        iv, x = self.iv, x0
        for k in range(iv.H):
            sv = self.svs[k if self.mode != "none" else 0]
            x = iv.emit(xs, k, x, sv.forward(x, iv.control(u, k), 1, self.n, self.method, iv.step(k), *self.tol))
        self.solve_ids = [sv.stats["solves"] for sv in self.svs]

    def backward(self, dout, need_p, out=None):
        iv, svs = self.iv, self.svs
        assert all(sv.stats["solves"] == i for sv, i in zip(svs, self.solve_ids)), \
            "%s: backward must run before the next %s of the same shape and mode with the same model" % (iv.api, iv.api)
        arena = self.func.device_handles()[0].arena if need_p else None
        carry, du_all, flat = None, None, None
        for k in range(iv.H - 1, -1, -1):            # dL/dx_{k+1} = dout[k+1] + what interval k+1 sends back
            sv = svs[k]
            gk = iv.grad_in(dout, k, carry)
            du, dy0 = sv.backward(gk.contiguous(), need_du=True, need_params=need_p, need_dy0=True)
            du_all = iv.add_du(du_all, k, du)
            carry = iv.grad_carry(dout, k, dy0)
            if need_p:
                fk = _reduce(arena, sv.accumulate_param_grads(arena, iv.slabs(arena, sv)))
                flat = fk if flat is None else flat + fk
        return dout[0] + carry, du_all, flat


def check_adjoint_chunk(api, adjoint, adjoint_chunk, chained=False):
    """``adjoint_chunk`` is a positive int or None, goes with ``adjoint=True`` only, and not with a backward that has no
    chunks (``chained``: rollout's dopri5)."""
    if adjoint_chunk is None:
        return
    if isinstance(adjoint_chunk, bool) or not isinstance(adjoint_chunk, int) or adjoint_chunk < 1:
        raise ValueError("%s: adjoint_chunk must be a positive int (output intervals per backward launch) or None; got %r"
                         % (api, adjoint_chunk))
    if not adjoint:
        raise ValueError("%s: adjoint_chunk goes with adjoint=True (the direct backward is one launch over the whole "
                         "horizon); got adjoint_chunk=%r with adjoint=False" % (api, adjoint_chunk))
    if chained:
        raise ValueError("%s: adjoint_chunk goes with method='euler' or 'rk4'; dopri5's backward is a chain of "
                         "one-interval adjoint solves, which has no chunks" % api)


class AdjointPlan:
    """What ``adjoint=True`` adds to a solve: per OUTPUT interval (a control interval of ``rollout``, [t[j-1], t[j]] of
    ``odeint_grid``) the fine steps of its backward solve, in the order they are applied from the interval's upper end
    (one step without ``step_size``; else ``ode_grid._sub_grid`` over [0, length]: the cut step falls at the lower
    end); whether the controls come one set per output interval with their gradient stacked (``rollout``) or one set
    for all with the gradient summed (``odeint_grid``); and the caller's ``adjoint_chunk``."""

    def __init__(self, steps, stacked, chunk=None, sub=False):
        self.steps, self.stacked, self.chunk, self.sub = tuple(tuple(s) for s in steps), stacked, chunk, sub
        self.H = len(self.steps)

    def run(self, lo, hi):
        """The fine intervals of the run over the output intervals lo <= k < hi, in ascending order (the launch walks
        them last to first): their steps, and the output interval whose upper end each one is (-1: none)."""
        hs, begin = [], []
        for k in range(lo, hi):
            hs += list(reversed(self.steps[k]))
            begin += [-1] * (len(self.steps[k]) - 1) + [k]
        return hs, begin

    def runs(self, chunk):
        """The runs of a backward in chunks of ``chunk`` output intervals, last run first: (lo, hi) each."""
        return [(max(0, hi - chunk), hi) for hi in range(self.H, 0, -chunk)]

    def pick_chunk(self, rows_limit, n, S):
        """The largest chunk (whole output intervals) none of whose runs has ``rows_limit`` stage rows or more."""
        if self.chunk is not None:
            return min(self.chunk, self.H)
        for chunk in range(self.H, 1, -1):
            if all(sum(len(self.steps[k]) for k in range(lo, hi)) * S * n < rows_limit for lo, hi in self.runs(chunk)):
                return chunk
        return 1


DW_ROWS_SLACK = 16 * 8      # per slab: the rows the weight-gradient ring requests past the end (mlp_dw16_kernels.hip)


def _dw_rows_limit(hid, n_slabs):
    """Rows one nlbac_mlp_bwd_weights launch takes for nets of width ``hid``: fewer than 2^29 elements per layer (up to
    112 units the launch refuses more; wider nets would fall from their 64-row-staged kernel, 256-wide tiles, to the
    older one)."""
    return (2 ** 29 - 1) // (hid if hid <= 112 else 256) - DW_ROWS_SLACK * n_slabs - 4


class _AdjTraj:
    """The one-launch backward of ``adjoint=True``: nothing of the forward is kept but the outputs the caller holds and
    the controls.  The forward is the direct path's in keep-mode "none" (its K / Y / G scratch dropped when it returns);
    the backward walks the horizon last to first in runs of whole output intervals — one ``nlbac_*_adj_traj`` launch per
    run, a carry row handing z = [y | a_x | a_c] from run to run — and, with parameter gradients, one
    ``nlbac_mlp_bwd_weights`` + ``nlbac_reduce_slabs`` per run over what the launch kept of every stage, the runs'
    flat gradients summed last run first.  Kept buffers are sized by the chunk, not by the horizon."""
    dx0_total = True

    def __init__(self, func, n, iv, method, plan, device):
        self.func, self.n, self.iv, self.method, self.plan, self.device = func, n, iv, method, plan, device
        self.S, self.beta, self.c_out = _tableau(method)
        self.ns = func.n_s
        self._arrays = {}

    def forward(self, x0, u, xs):
        self.u = u
        self.Direct(self.func, self.n, self.iv, self.method, "none", self.device).forward(x0, u, xs)

    def _run_arrays(self, lo, hi):
        a = self._arrays.get((lo, hi))
        if a is None:      # steps and markers twice: on the device for the kernel, in host memory for the launcher's checks
            hs, begin = self.plan.run(lo, hi)
            a = self._arrays[(lo, hi)] = (torch.tensor(hs, dtype=torch.float32, device=self.device), fptr(*hs),
                                          torch.tensor(begin, dtype=torch.int32, device=self.device),
                                          (C.c_int * len(begin))(*begin), len(hs))
        return a

    def backward(self, dout, need_p, out):
        n, ns, nc, S, plan, dev = self.n, self.ns, self.nc, self.S, self.plan, self.device
        W = 2 * ns + nc
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        limit = min(self.rows_limit(), 2 ** 31) if need_p else 2 ** 31
        chunk = self.chunk_used = plan.pick_chunk(limit, n, S)
        runs = plan.runs(chunk)
        carry = z(n, W)
        du = z(plan.H, n, nc) if plan.stacked else z(n, nc)
        stride = n * nc if plan.stacked else 0
        rows_max = max(self._run_arrays(lo, hi)[4] for lo, hi in runs) * S * n
        keep = self.keep_buffers(z, rows_max) if need_p else None
        flat = None
        for lo, hi in runs:
            hs_d, hs_h, bg_d, bg_h, N = self._run_arrays(lo, hi)
            self.launch(n, N, plan.H, hs_d.data_ptr(), hs_h, bg_d.data_ptr(), bg_h, out.data_ptr(), out.shape[2],
                        dout.data_ptr(), self.u.data_ptr(), stride, du.data_ptr(), stride, carry.data_ptr(),
                        1 if hi == plan.H else 0, keep, N * S * n)
            if need_p:
                fk = self.weight_grads(keep, N * S * n)
                flat = fk if flat is None else flat + fk
        return dout[0] + carry[:, ns:2 * ns], du, flat


class AffineAdjTraj(_AdjTraj):
    """``_AdjTraj`` of the control-affine NODE: ``nlbac_node_adj_traj``."""
    Direct = AffineTraj

    @staticmethod
    def ok(func):
        f, g = func.device_handles()
        return _lib.load().nlbac_node_adj_traj_ok(C.byref(f.desc), C.byref(g.desc)) == 1

    def __init__(self, func, n, iv, method, plan, device):
        _AdjTraj.__init__(self, func, n, iv, method, plan, device)
        self.f, self.g = func.device_handles()
        self.nc = func.n_u

    def rows_limit(self):
        return _dw_rows_limit(max(self.f.hid, self.g.hid), self.f.arena.n_slabs)

    def keep_buffers(self, z, rows):
        f, g, ns, nu = self.f, self.g, self.ns, self.nc
        return dict(ZS=z(rows, 2 * ns + nu), dK=z(rows, ns), dG=z(rows, ns * nu), acts_f=z((f.n_layers - 1) * rows * f.hid),
                    acts_g=z((g.n_layers - 1) * rows * g.hid), dz_f=z((f.n_layers - 1) * rows * f.hid),
                    dz_g=z((g.n_layers - 1) * rows * g.hid))

    def launch(self, n, N, H, hs, hs_host, begin, begin_host, out, out_ld, dout, u, u_stride, du, du_stride, carry, top,
               keep, rows):
        k = keep or {}
        _lib.call("nlbac_node_adj_traj", C.byref(self.f.desc), C.byref(self.g.desc), n, N, H, self.S, self.beta, self.c_out,
                  hs, hs_host, begin, begin_host, out, out_ld, dout, u, u_stride, du, du_stride, carry, top,
                  _ptr(k.get("ZS")), _ptr(k.get("dK")), _ptr(k.get("dG")), _ptr(k.get("acts_f")), rows * self.f.hid,
                  _ptr(k.get("acts_g")), rows * self.g.hid, _ptr(k.get("dz_f")), _ptr(k.get("dz_g")), stream_ptr())

    def weight_grads(self, k, rows):
        # layer 0's input rows are the y columns of the kept z = [y | a_x | a_c] rows
        return _affine_weight_grads(self.f, self.g, k["ZS"].data_ptr(), 2 * self.ns + self.nc, (k["dK"], k["dG"]),
                                    (k["acts_f"].data_ptr(), k["acts_g"].data_ptr()),
                                    (rows * self.f.hid, rows * self.g.hid), (k["dz_f"], k["dz_g"]), rows, self.device)


class ConcatAdjTraj(_AdjTraj):
    """``_AdjTraj`` of the single-net NODE (normalised or not): ``nlbac_concat_adj_traj``."""
    Direct = ConcatTraj

    @staticmethod
    def ok(func):
        return _lib.load().nlbac_concat_adj_traj_ok(C.byref(func.device_handles()[0].desc)) == 1

    def __init__(self, func, n, iv, method, plan, device):
        _AdjTraj.__init__(self, func, n, iv, method, plan, device)
        self.net = func.device_handles()[0]
        self.nc = func.n_carry
        self.norm = func.norm_device() if getattr(func, "normalized", False) else None

    def rows_limit(self):
        return _dw_rows_limit(self.net.hid, self.net.arena.n_slabs)

    def keep_buffers(self, z, rows):
        net = self.net
        return dict(Xin=z(rows, net.in_dim), Ay=z(rows, self.ns), acts=z((net.n_layers - 1) * rows * net.hid),
                    dz=z((net.n_layers - 1) * rows * net.hid))

    def launch(self, n, N, H, hs, hs_host, begin, begin_host, out, out_ld, dout, u, u_stride, du, du_stride, carry, top,
               keep, rows):
        k = keep or {}
        _lib.call("nlbac_concat_adj_traj", C.byref(self.net.desc), n, N, H, self.S, self.beta, self.c_out, hs, hs_host,
                  begin, begin_host, out, out_ld, dout, u, u_stride, du, du_stride, carry, top, _ptr(self.norm),
                  _ptr(k.get("Xin")), _ptr(k.get("Ay")), _ptr(k.get("acts")), rows * self.net.hid, _ptr(k.get("dz")),
                  stream_ptr())

    def weight_grads(self, k, rows):
        return _concat_weight_grads(self.net, k["Xin"].data_ptr(), self.net.in_dim, k["Ay"], k["acts"].data_ptr(),
                                    rows * self.net.hid, k["dz"], rows, self.device)


def adj_traj_class(func):
    return AffineAdjTraj if func.affine else ConcatAdjTraj


class ChainSubAdjoint:
    """The chained path of ``adjoint=True`` with ``step_size``: the forward is the chained forward without gradients;
    the backward solves every output interval backwards on its own fine grid with one ``nlbac_*_adj_step`` launch per
    fine step (``ode_adjoint.AffineAdjoint.adjoint_interval``) on one solver, cached on the model under a key of its
    own.  Its dx0 and controls' gradient are the one-launch path's bit for bit."""
    dx0_total = True

    def __init__(self, func, n, iv, method, plan, atol, rtol):
        self.func, self.n, self.iv, self.method, self.plan, self.tol = func, n, iv, method, plan, (atol, rtol)

    def forward(self, x0, u, xs):
        self.u = u
        Chain(self.func, self.n, self.iv, self.method, "none", *self.tol).forward(x0, u, xs)

    def backward(self, dout, need_p, out):
        func, plan, ns = self.func, self.plan, self.func.n_s
        sv = func.__dict__.get("_grid_adjoint_solver")
        if sv is None:
            sv = func.__dict__["_grid_adjoint_solver"] = traj_class(func).Solver(func, func.device_handles()[0].arena.device)
            sv.adjoint = True
        par = sv.adjoint_grid_begin(self.n, self.method, need_p, *self.tol)
        carry, du_all = None, None
        for k in range(plan.H - 1, -1, -1):
            a = dout[k + 1] if carry is None else (dout[k + 1] + carry)
            du, dy0 = sv.adjoint_interval(out[k + 1][:, :ns].contiguous(), a.contiguous(),
                                          self.u[k] if plan.stacked else self.u, self.method, plan.steps[k], par)
            if plan.stacked:
                if du_all is None:
                    du_all = torch.empty(plan.H, *du.shape, dtype=torch.float32, device=du.device)
                du_all[k].copy_(du)
            else:
                du_all = du.clone() if du_all is None else du_all + du
            carry = dy0.clone()
        return dout[0] + carry, du_all, par["th0"].clone() if need_p else None


def solve_adjoint(func, iv, method, mode, one_launch, plan, x0, u, xs, atol=1e-7, rtol=1e-5):
    """``solve`` under ``adjoint=True``: the same forward values, nothing kept for the backward but what the caller
    holds — returns an object whose ``backward(dout, need_p, out=out)`` takes the forward's stored outputs
    (plan.H + 1, n, >= n_s: the state in the first n_s columns) and gives what ``solve``'s does, or None without
    gradients.  ``one_launch``: the direct path's answer; the adjoint launch must serve the nets as well."""
    n = x0.shape[0]
    if mode == "none":
        solve(func, iv, method, "none", one_launch, x0, u, xs, atol, rtol)
        return None
    if one_launch and adj_traj_class(func).ok(func):
        kept = adj_traj_class(func)(func, n, iv, method, plan, x0.device)
    elif plan.sub:
        kept = ChainSubAdjoint(func, n, iv, method, plan, atol, rtol)
    else:      # (dopri5, shapes the kernels refuse, ``ONE_LAUNCH = False``: H one-interval ``odeint_adjoint`` solves)
        kept = Chain(func, n, iv, method, mode, atol, rtol, adjoint=True)
    kept.forward(x0, u, xs)
    return kept


def solve(func, iv, method, mode, one_launch, x0, u, xs, atol=1e-7, rtol=1e-5):
    """Solve the intervals ``iv`` from ``x0`` (n, n_s) under the controls ``u`` into ``xs`` (iv.n_out, n, n_s) — H, one
    output per interval, unless the intervals say otherwise — in one launch (``one_launch``: the caller asked
    ``traj_class(func).ok``) or chained.  Returns what ``mode`` keeps: an object whose
    ``backward(dout (iv.n_out + 1, n, n_s), need_p)`` gives (dx0, the controls' gradient, the flat parameter gradient or None),
    or None without gradients."""
    n = x0.shape[0]
    if isinstance(iv, TileSteps):      # (dopri5 under tile-local step control: one launch, no chained form)
        kept = AffineTileDopri(func, n, iv, mode, atol, rtol, x0.device)
    else:
        kept = traj_class(func)(func, n, iv, method, mode, x0.device) if one_launch else Chain(func, n, iv, method, mode, atol, rtol)
    kept.forward(x0, u, xs)
    return kept if mode != "none" else None
