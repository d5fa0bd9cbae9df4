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
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import fptr
from .arena import bwd_weights, io_array, mlp_array, stream_ptr
from .ode_consts import TABLEAU, env_switch
from .odeint import AffineNodeSolver, ConcatNodeSolver

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
    grad_on = torch.is_grad_enabled()
    if grad_on and any(p.requires_grad for p in params):
        mode = "params"
    elif grad_on and (x0.requires_grad or controls.requires_grad):
        mode = "inputs"
    else:
        mode = "none"
    func.refresh_device_weights()
    return _RolloutFunction.apply(func, method, dt, float(atol), float(rtol), mode, x0, controls, *params)


def _one_launch_ok(func, method):
    if not (ONE_LAUNCH and method in ("euler", "rk4")):
        return False
    if not func.affine:
        return _lib.load().nlbac_concat_rk_traj_ok(C.byref(func.device_handles()[0].desc)) == 1
    f, g = func.device_handles()
    return _lib.load().nlbac_node_rk_traj_ok(C.byref(f.desc), C.byref(g.desc)) == 1


def _chain_solvers(func, mode, H, key="_rollout_solvers"):
    """Solvers of the chained path, cached on the model (apart from ``odeint``'s and any agent task's): one per interval
    when a backward follows (each keeps its interval's state), one for all intervals otherwise.  ``key``: the cache's
    name on the model (``ode_grid.odeint_grid`` keeps solvers of its own)."""
    cache = func.__dict__.setdefault(key, {})
    lst = cache.setdefault(mode, [])
    need = 1 if mode == "none" else H
    if len(lst) < need:
        dev = func.device_handles()[0].arena.device
        for _ in range(need - len(lst)):
            sv = (AffineNodeSolver if func.affine else ConcatNodeSolver)(func, dev)
            sv.keep_acts = mode != "inputs"      # (no grad: the same kernels as odeint's solver; nothing is read back)
            lst.append(sv)
    return lst


def _tableau(method):
    tab = TABLEAU[method]
    S = len(tab["c_sol"])
    beta = [0.0] * (S * S)
    for i, r in enumerate(tab["beta"]):
        for j, v in enumerate(r):
            beta[(i + 1) * S + j] = v
    return S, fptr(*beta), fptr(*tab["c_sol"])


class _Traj:
    """Device buffers of one one-launch rollout: step-major [k][stage][row] over H * S stages."""

    def __init__(self, func, n, H, method, mode, device):
        f, g = func.device_handles()
        self.f, self.g = f, g
        self.ns, self.nu = func.n_s, func.n_u
        self.S, self.beta, self.c_out = _tableau(method)
        self.n, self.H = n, H
        HS = H * self.S
        z = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=device)
        self.K, self.Y, self.G = z(HS, n, self.ns), z(HS, n, self.ns), z(HS, n, self.ns * self.nu)
        self.rows = mode == "params"
        words = mode == "inputs" or (self.rows and env_switch("fit_words"))
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

    def ptr(self, i):
        return self.acts[i].data_ptr() if self.acts[i] is not None else None


class _ConcatTraj:
    """Device buffers of one one-launch rollout of the single-net NODE, step-major [k][stage][row] over H * S stages:
    nothing without gradients, the three layers' mask words for input gradients, activation rows and the stage-input
    rows layer 0 saw ([Y_st | c_k], normalised when the net is) for parameter gradients."""

    def __init__(self, func, n, H, method, mode, device):
        self.net = func.device_handles()[0]
        self.ns, self.nc = func.n_s, func.n_carry
        self.S, self.beta, self.c_out = _tableau(method)
        self.n, self.H = n, H
        self.norm = func.norm_device() if getattr(func, "normalized", False) else None
        HS, nw = H * self.S, self.net.n_layers - 1
        self.bits = 1 if mode == "inputs" else 0
        self.acts, self.ls, self.Xin = None, 0, None
        if mode == "inputs":
            self.acts, self.ls = torch.empty(nw * HS * n * 4, dtype=torch.int32, device=device), HS * n * 4
        elif mode == "params":
            self.acts = torch.empty(nw, HS * n, self.net.hid, dtype=torch.float32, device=device)
            self.ls = HS * n * self.net.hid
            self.Xin = torch.empty(HS * n, self.net.in_dim, dtype=torch.float32, device=device)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _RolloutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, method, dt, atol, rtol, mode, x0, controls, *params):
        H, n, ns = controls.shape[0], x0.shape[0], func.n_s
        x0 = x0.detach().contiguous()
        u = controls.detach().contiguous()
        out = torch.empty(H + 1, n, ns, dtype=torch.float32, device=x0.device)
        out[0].copy_(x0)
        ctx.func, ctx.mode, ctx.n_params = func, mode, len(params)
        if _one_launch_ok(func, method) and not func.affine:
            tj = _ConcatTraj(func, n, H, method, mode, x0.device)
            _lib.call("nlbac_concat_rk_traj_fwd", C.byref(tj.net.desc), x0.data_ptr(), u.data_ptr(), n, H, tj.S, tj.beta,
                      tj.c_out, dt, out[1].data_ptr(), _ptr(tj.Xin), _ptr(tj.acts), tj.ls, tj.bits, _ptr(tj.norm),
                      stream_ptr())
            ctx.path = ("ctraj", tj, dt) if mode != "none" else None
            return out
        if _one_launch_ok(func, method):
            tj = _Traj(func, n, H, method, mode, x0.device)
            _lib.call("nlbac_node_rk_traj_fwd", C.byref(tj.f.desc), C.byref(tj.g.desc), x0.data_ptr(), u.data_ptr(), n,
                      H, tj.S, tj.beta, tj.c_out, dt, out[1].data_ptr(), tj.K.data_ptr(), tj.Y.data_ptr(),
                      tj.G.data_ptr(), tj.ptr(0), tj.ls[0], tj.ptr(1), tj.ls[1], tj.bits, stream_ptr())
            ctx.path = ("traj", tj, u, dt) if mode != "none" else None
            return out
        svs = _chain_solvers(func, mode, H)
        for k in range(H):
            sv = svs[k if mode != "none" else 0]
            out[k + 1].copy_(sv.forward(out[k], u[k], 1, n, method, dt, atol, rtol))
        if mode != "none":
            ctx.path = ("chain", svs[:H], [sv.stats["solves"] for sv in svs[:H]])
        else:
            ctx.path = None
        return out

    @staticmethod
    def backward(ctx, dout):
        func, path = ctx.func, ctx.path
        assert path is not None, "rollout: nothing was kept for a backward (the forward ran without gradients)"
        dout = dout.float().contiguous()
        need_p = ctx.mode == "params" and any(ctx.needs_input_grad[8:])
        if path[0] == "ctraj":
            dx0, du, flat = _concat_traj_backward(func, path[1], path[2], dout, need_p)
        elif path[0] == "traj":
            dx0, du, flat = _traj_backward(func, path[1], path[2], path[3], dout, need_p)
        else:
            dx0, du, flat = _chain_backward(func, path[1], path[2], dout, need_p)
        gp = [None] * ctx.n_params
        if need_p:
            arena = func.device_handles()[0].arena
            gp = []
            for p in func.parameters():
                off = arena.offset_of[id(p)]
                gp.append(flat[off:off + p.numel()].view(p.shape))
        return (None, None, None, None, None, None, dx0 if ctx.needs_input_grad[6] else None,
                du if ctx.needs_input_grad[7] else None, *gp)


def _reduce(arena, used):
    flat = torch.empty(arena.n, dtype=torch.float32, device=arena.device)
    _lib.call("nlbac_reduce_slabs", flat.data_ptr(), arena.grad.data_ptr(), used, arena.n, arena.n, stream_ptr())
    return flat


def _chain_backward(func, svs, solve_ids, dout, need_p):
    assert all(sv.stats["solves"] == i for sv, i in zip(svs, solve_ids)), \
        "rollout: backward must run before the next rollout of the same shape and mode with the same model"
    H = len(svs)
    n, nc = dout.shape[1], svs[0].n_u
    du_all = torch.empty(H, n, nc, dtype=torch.float32, device=dout.device)
    arena = func.device_handles()[0].arena if need_p else None
    carry, flat = None, None
    for k in range(H - 1, -1, -1):            # dL/dx_{k+1} = dout[k+1] + what interval k+1 sends back
        sv = svs[k]
        gk = dout[k + 1] if carry is None else (dout[k + 1] + carry)
        du, dy0 = sv.backward(gk.contiguous(), need_du=True, need_params=need_p, need_dy0=True)
        du_all[k].copy_(du)
        carry = dy0.clone()
        if need_p:
            n_steps = max(1, len(sv.ctx.get("steps") or [None]))
            fk = _reduce(arena, sv.accumulate_param_grads(arena, max(1, arena.n_slabs // n_steps)))
            flat = fk if flat is None else flat + fk
    return dout[0] + carry, du_all, flat


def _traj_backward(func, tj, u, dt, dout, need_p, hs=None):
    """``hs`` (``ode_grid``): (device array, host array) of the intervals' step sizes in place of ``dt`` — the time-grid
    launch, whose ``u`` (n, n_u) is every interval's and whose ``du`` (n, n_u) is summed over the intervals."""
    n, H, S, HS = tj.n, tj.H, tj.S, tj.H * tj.S
    dev = dout.device
    z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dx0, du = z(n, tj.ns), (z(H, n, tj.nu) if hs is None else z(n, tj.nu))
    name, step = ("nlbac_node_rk_traj_bwd", (dt,)) if hs is None else ("nlbac_node_rk_grid_bwd", (hs[0].data_ptr(), hs[1]))
    dK = dG = dz_f = dz_g = None
    if need_p:
        dK, dG = z(HS, n, tj.ns), z(HS, n, tj.ns * tj.nu)
        dz_f, dz_g = z(tj.f.n_layers - 1, HS * n, tj.f.hid), z(tj.g.n_layers - 1, HS * n, tj.g.hid)
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.call(name, C.byref(tj.f.desc), C.byref(tj.g.desc), u.data_ptr(), n, H, S, tj.beta,
              tj.c_out, *step, tj.G.data_ptr(), tj.ptr(0), tj.ls[0], tj.ptr(1), tj.ls[1], tj.bits, dout.data_ptr(),
              dx0.data_ptr(), du.data_ptr(), p(dK), p(dG), p(dz_f), p(dz_g), stream_ptr())
    flat = None
    if need_p:      # every stage of every interval as ONE batch of H * S * n rows through the weight-gradient launch
        arena = func.device_handles()[0].arena
        io = io_array(2)
        for i, (net, dy, ld, dz) in enumerate(((tj.f, dK, tj.ns, dz_f), (tj.g, dG, tj.ns * tj.nu, dz_g))):
            io[i].x0, io[i].x0_dim, io[i].x0_ld = tj.Y.data_ptr(), tj.ns, tj.ns
            io[i].dy, io[i].dy_ld = dy.data_ptr(), ld
            io[i].acts, io[i].acts_ls = tj.ptr(i), tj.ls[i]
            io[i].dz = dz.data_ptr()
            io[i].grad = arena.grad.data_ptr()
        bwd_weights(mlp_array([tj.f.desc, tj.g.desc]), io, 2, HS * n, arena.n_slabs, arena.n, dev)
        flat = _reduce(arena, arena.n_slabs)
    return dx0, du, flat


def _concat_traj_backward(func, tj, dt, dout, need_p, hs=None):
    """``hs``: as in ``_traj_backward`` (the carried columns' gradient (n, n_c) summed over the intervals)."""
    n, H, S, HS = tj.n, tj.H, tj.S, tj.H * tj.S
    dev = dout.device
    z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dx0, du = z(n, tj.ns), (z(H, n, tj.nc) if hs is None else z(n, tj.nc))
    name, step = ("nlbac_concat_rk_traj_bwd", (dt,)) if hs is None else ("nlbac_concat_rk_grid_bwd", (hs[0].data_ptr(), hs[1]))
    dK = dz = None
    if need_p:
        dK, dz = z(HS * n, tj.ns), z(tj.net.n_layers - 1, HS * n, tj.net.hid)
    _lib.call(name, C.byref(tj.net.desc), n, H, S, tj.beta, tj.c_out, *step, tj.acts.data_ptr(), tj.ls,
              tj.bits, _ptr(tj.norm), dout.data_ptr(), dx0.data_ptr(), du.data_ptr(), _ptr(dK), _ptr(dz), stream_ptr())
    flat = None
    if need_p:      # every stage of every interval as ONE batch of H * S * n rows: layer 0's input is the kept Xin row
        arena = tj.net.arena
        io = io_array(1)
        io[0].x0, io[0].x0_dim, io[0].x0_ld = tj.Xin.data_ptr(), tj.net.in_dim, tj.net.in_dim
        io[0].dy, io[0].dy_ld = dK.data_ptr(), tj.ns
        io[0].acts, io[0].acts_ls = tj.acts.data_ptr(), tj.ls
        io[0].dz = dz.data_ptr()
        io[0].grad = arena.grad.data_ptr()
        bwd_weights(mlp_array([tj.net.desc]), io, 1, HS * n, arena.n_slabs, arena.n, dev)
        flat = _reduce(arena, arena.n_slabs)
    return dx0, du, flat
