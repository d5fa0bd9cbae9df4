"""What ``rollout`` and ``ode_grid.odeint_grid`` share: a NODE solved over H intervals as one autograd node.

  * the intervals (``EqualSteps``: one ``dt`` and a control per interval, ``rollout``; ``GridSteps``: a step per
    interval and one set of controls, ``odeint_grid``; ``SubGridSteps``: the fine intervals of ``odeint_grid`` under
    ``step_size``, whose output points are interpolated; ``HeldSteps``: the fine intervals of ``rollout`` under
    ``step_size``, a control held over each m of them): the entry points' infix, their step arguments, what the
    controls' gradient looks like, where the outputs and their gradients meet the intervals;
  * what a solve keeps and how its backward becomes gradients, one class per path — ``AffineTraj`` / ``ConcatTraj`` (one
    launch forward, one backward, + the weight-gradient launch over all H * stages * rows) and ``Chain`` (H one-interval
    solves on the existing solvers) — each with ``forward(x0, u, xs)`` and ``backward(dout, need_p)``; ``solve`` picks.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import fptr
from .arena import bwd_weights, io_array, mlp_array, stream_ptr
from .ode_consts import TABLEAU, env_switch
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
    tab = TABLEAU[method]
    S = len(tab["c_sol"])
    beta = [0.0] * (S * S)
    for i, r in enumerate(tab["beta"]):
        for j, v in enumerate(r):
            beta[(i + 1) * S + j] = v
    return S, fptr(*beta), fptr(*tab["c_sol"])


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _reduce(arena, used):
    flat = torch.empty(arena.n, dtype=torch.float32, device=arena.device)
    _lib.call("nlbac_reduce_slabs", flat.data_ptr(), arena.grad.data_ptr(), used, arena.n, arena.n, stream_ptr())
    return flat


def param_grads(func, flat):
    """The flat arena gradient as one view per parameter, in ``func.parameters()``'s order."""
    arena = func.device_handles()[0].arena
    return [flat[arena.offset_of[id(p)]:arena.offset_of[id(p)] + p.numel()].view(p.shape) for p in func.parameters()]


class AffineTraj:
    """Device buffers of one one-launch solve of the control-affine NODE: step-major [k][stage][row] over H * S stages."""
    Solver = AffineNodeSolver

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
        words = mode == "inputs" or (mode == "params" and env_switch("fit_words"))
        self.bits = 0 if mode == "none" else (1 if mode == "inputs" else (2 if words else 0))
        self.acts, self.ls = [None, None], [0, 0]
        if mode != "none":
            for i, net in enumerate((f, g)):
                nw = net.n_layers - 1
                if mode == "inputs":                       # words in place of the rows
                    self.acts[i], self.ls[i] = z(nw * HS * n * 4, dtype=torch.int32), HS * n * 4
                else:                                      # rows [layer][HS n][hid], then (bits 2) words [layer][HS n][4]
                    self.acts[i] = z(nw * HS * n * (net.hid + (4 if words else 0)))
                    self.ls[i] = HS * n * net.hid

    def forward(self, x0, u, xs):
        self.u = u
        _lib.call("nlbac_node_rk_%s_fwd" % self.iv.infix, C.byref(self.f.desc), C.byref(self.g.desc), x0.data_ptr(),
                  u.data_ptr(), self.n, self.iv.launch_H, self.S, self.beta, self.c_out, *self.iv.step_args(),
                  xs.data_ptr(), self.K.data_ptr(), self.Y.data_ptr(), self.G.data_ptr(), _ptr(self.acts[0]), self.ls[0],
                  _ptr(self.acts[1]), self.ls[1], self.bits, stream_ptr())

    def backward(self, dout, need_p):
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
        arena = self.f.arena
        io = io_array(2)
        for i, (dy, ld, dz) in enumerate(((dK, self.ns, dz_f), (dG, self.ns * self.nu, dz_g))):
            io[i].x0, io[i].x0_dim, io[i].x0_ld = self.Y.data_ptr(), self.ns, self.ns
            io[i].dy, io[i].dy_ld = dy.data_ptr(), ld
            io[i].acts, io[i].acts_ls = _ptr(self.acts[i]), self.ls[i]
            io[i].dz = dz.data_ptr()
            io[i].grad = arena.grad.data_ptr()
        bwd_weights(mlp_array([self.f.desc, self.g.desc]), io, 2, HS * n, arena.n_slabs, arena.n, dev)
        return dx0, du, _reduce(arena, arena.n_slabs)


class ConcatTraj:
    """Device buffers of one one-launch solve of the single-net NODE, step-major [k][stage][row] over H * S stages:
    nothing without gradients, the three layers' mask words for input gradients, activation rows and the stage-input
    rows layer 0 saw ([Y_st | c_k], normalised when the net is) for parameter gradients."""
    Solver = ConcatNodeSolver

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

    def backward(self, dout, need_p):
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
        arena = self.net.arena
        io = io_array(1)
        io[0].x0, io[0].x0_dim, io[0].x0_ld = self.Xin.data_ptr(), self.net.in_dim, self.net.in_dim
        io[0].dy, io[0].dy_ld = dK.data_ptr(), self.ns
        io[0].acts, io[0].acts_ls = self.acts.data_ptr(), self.ls
        io[0].dz = dz.data_ptr()
        io[0].grad = arena.grad.data_ptr()
        bwd_weights(mlp_array([self.net.desc]), io, 1, HS * n, arena.n_slabs, arena.n, dev)
        return dx0, du, _reduce(arena, arena.n_slabs)


def traj_class(func):
    """The one-launch path of ``func``'s NODE form (the one place that asks which form it is)."""
    return AffineTraj if func.affine else ConcatTraj


class Chain:
    """The chained path: H one-interval solves on the existing solvers, cached on the model under the intervals'
    ``solvers_key`` (apart from ``odeint``'s and any agent task's): one solver per interval when a backward follows (each
    keeps its interval's state), one for all intervals otherwise."""

    def __init__(self, func, n, iv, method, mode, atol, rtol):
        self.func, self.n, self.iv, self.method, self.mode, self.tol = func, n, iv, method, mode, (atol, rtol)
        lst = func.__dict__.setdefault(iv.solvers_key, {}).setdefault(mode, [])
        for _ in range((1 if mode == "none" else iv.H) - len(lst)):
            sv = traj_class(func).Solver(func, func.device_handles()[0].arena.device)
            sv.keep_acts = mode != "inputs"      # (no grad: the same kernels as odeint's solver; nothing is read back)
            lst.append(sv)
        self.svs = lst[:iv.H]

    def forward(self, x0, u, xs):
        iv, x = self.iv, x0
        for k in range(iv.H):
            sv = self.svs[k if self.mode != "none" else 0]
            x = iv.emit(xs, k, x, sv.forward(x, iv.control(u, k), 1, self.n, self.method, iv.step(k), *self.tol))
        self.solve_ids = [sv.stats["solves"] for sv in self.svs]

    def backward(self, dout, need_p):
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


def solve(func, iv, method, mode, one_launch, x0, u, xs, atol=1e-7, rtol=1e-5):
    """Solve the intervals ``iv`` from ``x0`` (n, n_s) under the controls ``u`` into ``xs`` (iv.n_out, n, n_s) — H, one
    output per interval, unless the intervals say otherwise — in one launch (``one_launch``: the caller asked
    ``traj_class(func).ok``) or chained.  Returns what ``mode`` keeps: an object whose
    ``backward(dout (iv.n_out + 1, n, n_s), need_p)`` gives (dx0, the controls' gradient, the flat parameter gradient or None),
    or None without gradients."""
    n = x0.shape[0]
    kept = traj_class(func)(func, n, iv, method, mode, x0.device) if one_launch else Chain(func, n, iv, method, mode, atol, rtol)
    kept.forward(x0, u, xs)
    return kept if mode != "none" else None
