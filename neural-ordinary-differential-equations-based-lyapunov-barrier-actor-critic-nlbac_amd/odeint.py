"""Batched IVP solve of the learned control-affine dynamics on ``t = [0, dt]``
and its exact (discretise-then-differentiate) backward — the device
replacement of the ``torchdiffeq.odeint`` call sites
``U/sac_cbf_clf/sac_cbf_clf.py:453,577`` and ``U/sac_cbf_clf/model.py:252``.

Solvers (same semantics as ``oracle/nlbac_oracle.odeint``):
  * ``euler``  one explicit Euler step over [0, dt] — the reference's setting
  * ``rk4``    one 3/8-rule step
  * ``dopri5`` Dormand–Prince 5(4), FSAL, one shared adaptive step per problem
               (RMS error norm over the whole (rows, n_s+n_u) tensor), result =
               4th-order interpolant at dt.  Step sizes carry no gradient.

Rows are ``P`` problems x ``rpp`` rows (e.g. primary and backup controller
actions on the same states).  Every stage costs one batched f_net/g_net
launch (``nlbac_mlp_fwd``) plus two per-row algebra kernels; the step-size
controller runs on the device and the host reads one 128-byte control block
per attempted step.

This module holds the solvers' construction, their launch wrappers, the forward dispatch with the fixed-step solvers,
the in- and out-maps, the discrete backward over a list of steps and the weight-gradient accumulation.  Beside it:
``ode_dopri`` (dopri5's adaptive step control: host-driven attempts, the device-driven chain, the per-problem fallback),
``ode_workspace`` (step slots and scratch buffers), ``ode_ctl`` (how the host reads the control block),
``ode_adjoint`` (the continuous adjoint), ``ode_consts`` (tableaus, control-block fields and environment switches).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import fptr
from .arena import bwd_weights, io_array, mlp_array, stream_ptr
from .ode_adjoint import AffineAdjoint, ConcatAdjoint
from .ode_consts import CTL_HUSED, DP_BETA, NORM_DEFER_ATTEMPT, TABLEAU, ctl_field_ptr, env_switch
from .ode_ctl import ControlBlockReader
from .ode_dopri import DopriDriver
from .ode_node import PackedSolve, SolveNode, _reduce
from .ode_workspace import SolverWorkspaces, _ConcatStepWS, _StepWS


class AffineNodeSolver(SolverWorkspaces, DopriDriver, AffineAdjoint):
    """odeint for ``dx/dt = f(x) + g(x) u`` with u constant over the step.  Step slots and scratch buffers:
    ``ode_workspace.SolverWorkspaces``; dopri5's step control: ``ode_dopri.DopriDriver``; the continuous adjoint:
    ``ode_adjoint.AffineAdjoint``."""
    STEP_WS = _StepWS
    OUT_MAP_IN_RK = True       # the RK kernels evaluate the owner's out-map (``set_out_map``) with the folded interpolation

    def __init__(self, node, device):
        self.node, self.f, self.g = node, node.f, node.g
        self.n_s, self.n_u = node.n_s, node.n_u
        # one nlbac_node_rk_fwd / _bwd launch per RK step instead of 3 launches per stage — when the fused backward's
        # LDS carve fits (4 tiles + both nets' first / last layers: up to 232-wide nets); wider ones run stage by stage
        self.fused = self._fused_fits(node.f, node.g)
        self._init_state(device)

    def _init_state(self, device):
        """Everything a solver keeps besides its field (both solver kinds).  Nothing here touches the device or the
        library: streams, pinned blocks and capability probes come at first use."""
        self.device = torch.device(device)
        self._init_workspaces()
        self._init_adjoint()
        self.ctx = None        # the state of the current solve (a dict, see ``forward_begin``)
        self.nfe = 0
        self._net_arr = None
        self._coefs = {}
        self.keep_acts = True  # False: backward never asks for weight gradients -> ReLU bit masks suffice
        self._children = {}    # per-problem solvers for batches whose problems diverge (dopri5), see ``_child``
        self.stats = dict(solves=0, single_step=0, multi_attempt=0, split=0)
        self.ctl = ControlBlockReader(self.device, self.stats)      # how the host reads dopri5's accept decisions
        self.before_wait = None   # the owner's hook, run before the host blocks on an accept decision (``_ctl_read``)
        self.comm = None       # nlbac_amd.parallel.DataParallel: global dopri5 error norms
        # > 1: every problem of a solve is cut into this many contiguous row groups, each an adaptive solve of its own
        # (own error norm, step sizes and accept decisions) — what a sample-sharded run with per-shard step control
        # (SAC_CBF_CLF.enable_data_parallel(step_control="shard")) computes on that many ranks, on one device
        self.row_groups = 1
        self.adjoint = False   # True: ``backward`` is the continuous adjoint (odeint_adjoint); the forward keeps nothing
        # True: a launch that keeps nothing runs the kernel instance of a solver that keeps activation rows (acts_bits 0)
        # although this solver's slots hold mask words only (keep_acts False) — that instance's sums, bit for bit, in
        # slots without rows (ode_dense.odeint_dense_adjoint)
        self.rows_sums = False
        self.device_loop = True   # dopri5 attempts as a device-driven chain (no host decision per attempt)
        self._chain_len = 1    # attempts the last chain solve needed = launches enqueued before the host first looks
        self._in_map, self._in_map_armed = None, False      # ``set_in_map``
        self._out_map = None                                # ``set_out_map``
        # A/B switches (ode_consts): the environment's value unless assigned before the first solve
        self.norm_defer = env_switch("norm_defer")
        self.norm_defer_attempt = NORM_DEFER_ATTEMPT
        self.interp_fold = env_switch("interp_fold")
        self.fit_words = env_switch("fit_words")
        # what the library says about the nets' kernels, asked once at first use
        self._words_ok = None      # nlbac_node_rk_mask_words == 4 for both nets (``_fit_words_on``)
        self._interp_ok = None     # nlbac_rk_interp_ok (``_rr_kernels``)

    @staticmethod
    def _fused_fits(f, g):
        pad = lambda x, m: (x + m - 1) // m * m
        ld = pad(max(f.hid, g.hid), 32) + 4
        sw = pad((f.out_dim + f.in_dim) * f.hid, 4) + pad((g.out_dim + g.in_dim) * g.hid, 4)
        lds = 4 * (4 * 32 * ld + 32 * 8 * 8 + 32 * (2 * 8 + 2 * 16 + 4 + 1 + 8 + 4) + sw)      # nlbac_node_rk_bwd's carve
        return lds <= 160 * 1024 - 64

    def _fit_words_on(self):
        """A solve whose backward wants weight gradients (the NODE fit: ``keep_acts``) keeps the activation rows AND the
        ReLU mask words (acts_bits 2) where the register-resident kernels serve both nets: the backward gates on the
        words instead of re-reading the rows, which only the weight gradients need.  ``fit_words = False``
        (NLBAC_FIT_WORDS=0): rows only, the backward gates on them — the cross-check."""
        if not (self.fused and self.keep_acts):
            return False
        if not self.fit_words:
            return False
        ok = self._words_ok
        if ok is None:
            lib, f, g = _lib.load(), C.byref(self.f.desc), C.byref(self.g.desc)
            ok = self._words_ok = lib.nlbac_node_rk_mask_words(f, g, 0) == 4 and lib.nlbac_node_rk_mask_words(f, g, 1) == 4
        return ok

    def reserve(self, n, P, method, steps=2):
        """Allocate the buffers of a solve on n rows / P problems ahead of time (the slot pool and, for a host-driven
        multi-problem dopri5 solve, the per-problem fallback solvers), so that the first multi-step or diverging solve
        of a run does not pay tens of milliseconds of allocation in the middle of training."""
        self._touch(n)
        P *= self.row_groups
        if method != "dopri5":
            S = len(TABLEAU[method]["c_sol"])
            self._step_ws(n, S, 0).bwd(self)
            return
        for idx in range(steps):
            self._step_ws(n, 7, idx).bwd(self)
        self.ctl.io(P)
        if P > 1 and not self._chain_ok(P, n // P):
            for p in range(P):
                self._child(p).reserve(n // P, 1, method, steps)

    # -- one field evaluation k = f(x) + g(x) u -----------------------------------
    def _nets(self):
        if self._net_arr is None:
            self._net_arr = mlp_array([self.f.desc, self.g.desc])
        return self._net_arr

    def _eval_io(self, x, g_out, acts_f=None, acts_g=None, ls_f=0, ls_g=0):
        io = io_array(2)
        ns, nu = self.n_s, self.n_u
        fout = self._buf("fout", x.shape[0], ns)
        for i, (y, ld, acts, ls) in enumerate(((fout, ns, acts_f, ls_f), (g_out, ns * nu, acts_g, ls_g))):
            io[i].x0, io[i].x0_dim, io[i].x0_ld = x.data_ptr(), ns, ns
            io[i].y, io[i].y_ld = y.data_ptr(), ld
            if acts is not None:
                io[i].acts, io[i].acts_ls = acts.data_ptr(), ls
        return io, fout

    def _eval(self, x, u, n, k_out, g_out, io=None):
        if io is None:
            io = self._eval_io(x, g_out)
        io, fout = io
        s = stream_ptr()
        _lib.call("nlbac_mlp_fwd", self._nets(), io, 2, n, s)
        _lib.call("nlbac_affine_combine_fwd", fout.data_ptr(), g_out.data_ptr(), u.data_ptr(), self.n_s, self.n_u, n,
                  k_out.data_ptr(), s)
        self.nfe += 1

    def _probe_eval(self, ytmp, u, n, ktmp, gtmp):
        """field evaluation outside the step workspaces (dopri5 initial-step probe), nothing saved"""
        pool = self._scratch.setdefault(self._cur_n, {})
        tio = pool.get(("tmp_io", n))
        if tio is None:
            tio = pool[("tmp_io", n)] = self._eval_io(ytmp, gtmp)
        self._eval(ytmp, u, n, ktmp, gtmp, tio)

    def _stage_eval(self, ws, st, u):
        n, S = ws.n, ws.S
        io = ws.io_fwd.get(st)
        if io is None:       # pointers are static per (workspace, stage): build the descriptors once
            f, g = self.f, self.g
            io = ws.io_fwd[st] = self._eval_io(ws.Y[st], ws.gout[st], ws.acts_f[:, st * n:], ws.acts_g[:, st * n:],
                                               S * n * f.hid, S * n * g.hid)
        self._eval(ws.Y[st], u, n, ws.K[st], ws.gout[st], io)

    def _beta(self, method):
        key = ("beta", method)
        b = self._coefs.get(key)
        if b is None:
            rows = TABLEAU[method]["beta"]
            S = len(rows) + 1
            flat = [0.0] * (S * S)
            for i, r in enumerate(rows):
                for j, v in enumerate(r):
                    flat[(i + 1) * S + j] = v
            b = self._coefs[key] = (fptr(*flat), S)
        return b

    def _rk_fused(self, ws, y0, u, P, rpp, method, st0, st1, h_host=None, h_dev=None, c_out=None, out=None,
                  c_err=None, err=None, save_acts=True, chain=None):
        """One launch for stages [st0, st1) of ``method`` on the step workspace ``ws`` (nlbac_node_rk_fwd)."""
        beta, S = self._beta(method)
        f, g = self.f, self.g
        n = P * rpp
        save_acts = save_acts and not self.adjoint       # (the adjoint re-computes every stage it differentiates)
        im = None
        if st0 == 0 and self.ctx.pop("in_map_pending", None):
            # first launch of the solve: it forms the initial state itself (set_in_map) and leaves it in y0
            m, im = self._in_map, _lib.InMap()
            im.kind, im.obs, im.obs_ld, im.l = m["kind"], m["obs"].data_ptr(), m["obs_ld"], m["l"]
            im.ps = m["ps"].data_ptr() if m["ps"] is not None else None
        _lib.call("nlbac_node_rk_fwd", C.byref(f.desc), C.byref(g.desc), y0.data_ptr(), u.data_ptr(), P, rpp,
                  st0, st1, S, beta, c_out, len(c_out) if c_out is not None else 0,
                  c_err, len(c_err) if c_err is not None else 0,
                  fptr(*h_host) if h_host is not None else None, h_dev, _lib.DOPRI_CTL if h_dev else 0,
                  ws.K.data_ptr(), ws.Y.data_ptr(), ws.gout.data_ptr(),
                  ws.acts_f.data_ptr() if save_acts else None, ws.S * n * ws.wf,
                  ws.acts_g.data_ptr() if save_acts else None, ws.S * n * ws.wg,
                  ws.acts_bits if save_acts else int(ws.bits and not self.rows_sums),
                  out.data_ptr() if out is not None else None, err.data_ptr() if err is not None else None,
                  C.byref(chain) if chain is not None else None, C.byref(im) if im is not None else None, stream_ptr())
        self.nfe += st1 - st0

    def _rk_fused_bwd(self, ws, u, P, rpp, method, first_eval, need_dy0, need_params, h_host, h_dev, h_stride, top_up,
                      du, last, chain=None, back_idx=0):
        """One launch for the backward of every evaluated stage of the step in ``ws`` (nlbac_node_rk_bwd)."""
        beta_arr, _ = self._beta(method)
        f, g, S = self.f, self.g, ws.S
        _lib.call("nlbac_node_rk_bwd", C.byref(f.desc), C.byref(g.desc), u.data_ptr(), ws.gout.data_ptr(), P, rpp,
                  S, 0 if first_eval else 1, S, 1 if need_dy0 else 0, beta_arr, h_host, h_dev, h_stride,
                  ws.acts_f.data_ptr(), S * ws.n * ws.wf, ws.acts_g.data_ptr(), S * ws.n * ws.wg,
                  ws.acts_bits, ws.dz_f.data_ptr() if need_params else None,
                  ws.dz_g.data_ptr() if need_params else None, ws.dG.data_ptr() if need_params else None,
                  ws.dK.data_ptr(), top_up.data_ptr() if top_up is not None else None, ws.dy0.data_ptr(), 1,
                  du.data_ptr() if du is not None else None, 0 if last else 1,
                  C.byref(chain) if chain is not None else None, back_idx, stream_ptr())

    def _combine(self, y0, K, n_k, coef, h, P, rpp, out):
        _lib.call("nlbac_rk_combine", y0.data_ptr() if y0 is not None else None, K.data_ptr(), n_k,
                  fptr(*coef), fptr(*h), None, 0, P, rpp, self.n_s, out.data_ptr(), stream_ptr())

    # -- forward ---------------------------------------------------------------
    def forward(self, y0, u, P, rpp, method, dt, atol=1e-7, rtol=1e-5):
        """y0: (P*rpp, n_s), u: (P*rpp, n_u) contiguous device tensors.
        Returns x(dt) (P*rpp, n_s) (a solver-owned buffer, valid until the next call)."""
        self.forward_begin(y0, u, P, rpp, method, dt, atol, rtol)
        return self.forward_finish()

    def forward_begin(self, y0, u, P, rpp, method, dt, atol=1e-7, rtol=1e-5):
        """Enqueue everything up to the first point where the host has to look at a result (dopri5: the
        accept/reject decision of the first attempted step); euler/rk4 run to completion.  No host sync."""
        n = P * rpp
        assert y0.shape == (n, self.n_s) and u.shape == (n, self.n_u)
        if self.row_groups > 1:
            assert rpp % self.row_groups == 0, "row_groups must divide the rows of a problem"
            P, rpp = P * self.row_groups, rpp // self.row_groups
        self._touch(n)
        self.stats["solves"] += 1
        self.ctx = dict(method=method, P=P, rpp=rpp, n=n, u=u, y0=y0, steps=[], t_end=float(dt), atol=atol,
                        rtol=rtol)
        if self._in_map_armed:
            self._in_map_armed = False
            self.ctx["in_map_pending"] = True          # (consumed by the solve's first launch, _rk_fused)
        if method in ("euler", "rk4"):
            tab = TABLEAU[method]
            S = len(tab["c_sol"])
            ws = self._step_ws(n, S, 0)
            h = [float(dt)] * P
            if self.fused:
                out = self._out_buf(n, ws.y1)
                self._rk_fused(ws, y0, u, P, rpp, method, 0, S, h_host=h, c_out=fptr(*tab["c_sol"]), out=out)
                self.ctx["steps"].append(dict(ws=ws, h=h, first=True))
                self.ctx["out"] = out
                return
            ws.Y[0].copy_(y0)
            for st in range(S):
                self._stage_eval(ws, st, u)
                if st + 1 < S:
                    self._combine(y0, ws.K, st + 1, tab["beta"][st], h, P, rpp, ws.Y[st + 1])
            self._combine(y0, ws.K, S, tab["c_sol"], h, P, rpp, ws.y1)
            self.ctx["steps"].append(dict(ws=ws, h=h, first=True))
            self.ctx["out"] = ws.y1
        elif method == "dopri5":
            self._dopri_begin(y0, u, P, rpp)
        else:
            raise ValueError("unknown solver %r" % (method,))

    def forward_finish(self, assume_single_step=False):
        """Complete the solve and return x(dt).  dopri5: reads the 128-byte/problem control block (one host
        sync) and continues with further attempts if the first step was rejected or stopped short of dt.
        ``assume_single_step``: skip the read (the caller has already checked ``first_step_done``) — this
        variant enqueues only device work with device-resident step size, so it can be hipGraph-captured."""
        if self.ctx["method"] != "dopri5":
            return self.ctx["out"]
        return self._dopri_finish(assume_single_step)

    # -- input map (nlbac_in_map) --------------------------------------------------------------------------------
    def set_in_map(self, kind, obs, obs_ld, l, ps=None):
        """The NEXT ``forward_begin``'s ``y0`` is an output: the solve's first launch forms the initial state from the
        owner's observation rows (kind 1: the Unicycle tasks' state map, ``ps`` receives the state's look-ahead point)
        and leaves it there.  Fused control-affine solver only (``fused``)."""
        assert self.fused, "set_in_map: the stage-by-stage path reads y0"
        self._in_map = dict(kind=kind, obs=obs, obs_ld=int(obs_ld), l=float(l), ps=ps)
        self._in_map_armed = True

    # -- output map (nlbac_out_map) ------------------------------------------------------------------------------
    def set_out_map(self, kind, l, p, dp=None, dp2=None):
        """The owner's per-row map of the solve's output (kind 1: planar look-ahead point, ``p`` (n, 2) receives it,
        ``dp`` / ``dp2`` hold its gradient at backward time).  Evaluated inside the dopri5 interpolation launches of the
        device-driven chain; ``out_mapped`` / ``backward(None)`` tell / let the owner skip its own launches.  Anywhere
        else (fixed-step methods, host-driven steps, the adjoint) the map is not applied and the owner launches it."""
        self._out_map = dict(kind=kind, l=float(l), p=p, dp=dp, dp2=dp2)

    @property
    def out_mapped(self):
        return bool(self.ctx.get("out_mapped"))

    def _out_map_fwd(self, n):
        m = self._out_map
        if m is None or m["p"].shape[0] != n or self.adjoint:
            return None
        om = _lib.OutMap()
        om.kind, om.l, om.p = m["kind"], m["l"], m["p"].data_ptr()
        return om

    def _out_map_bwd(self, n):
        m = self._out_map
        if m is None or m["dp"] is None or not self.ctx.get("out_mapped"):
            return None
        om = _lib.OutMap()
        om.kind, om.l, om.dp = m["kind"], m["l"], m["dp"].data_ptr()
        om.dp2 = m["dp2"].data_ptr() if m["dp2"] is not None else None
        om.x = self.ctx["out"].data_ptr()
        return om

    def _interp_nets(self):
        return C.byref(self.f.desc), C.byref(self.g.desc)

    # -- backward --------------------------------------------------------------
    def backward(self, dout, need_du=True, need_params=False, need_dy0=False):
        """dout: (n, n_s).  Returns (du or None, dy0 or None).  With
        ``need_params`` the pre-activation grads of every stage are kept for
        ``accumulate_param_grads``."""
        ctx = self.ctx
        if self.adjoint:
            return self.backward_adjoint(dout, need_du, need_params, need_dy0)
        if ctx.get("chain"):
            return self._backward_chain(dout, need_du, need_params, need_dy0)
        if ctx.get("split"):
            return self._backward_split(dout, need_du, need_params, need_dy0)
        P, rpp, n, u, method = ctx["P"], ctx["rpp"], ctx["n"], ctx["u"], ctx["method"]
        ns, nu = self.n_s, self.n_u
        s = stream_ptr()
        assert not (need_params and not self.keep_acts), "this solver keeps ReLU masks only (keep_acts=False)"
        du = self._buf("du", n, nu) if need_du else None
        if du is not None and not self.fused:
            du.zero_()           # (the fused kernel overwrites du on the first step it processes)
        steps = ctx["steps"]
        dy_carry = None          # grad wrt the y1 of the step being processed
        dk_carry = None          # grad wrt f1 (=K[6]) of that step, from the next step's FSAL stage 0
        for si in range(len(steps) - 1, -1, -1):
            step = steps[si]
            ws = step["ws"].bwd(self)
            S = ws.S
            dev = step.get("dev", False)       # step size lives in the device control block
            h_host = None if dev else fptr(*step["h"])
            h_dev = ctl_field_ptr(self._ctl(P).data_ptr(), CTL_HUSED) if dev else None
            h_stride = _lib.DOPRI_CTL if dev else 0
            last = si == len(steps) - 1
            if not (method == "dopri5" and last):
                ws.dK.zero_()              # (the interpolant's backward assigns every stage of dK itself)
            if method == "dopri5":
                beta, first_eval = DP_BETA, step["first"]
                if last:
                    _lib.call("nlbac_dopri_interp_bwd", dout.data_ptr(), h_host, None if dev else fptr(*step["x"]),
                              self._ctl(P).data_ptr() if dev else None, P, rpp, ns,
                              ws.dy0.data_ptr(), ws.dy1.data_ptr(), ws.dK.data_ptr(), 0, None, s)
                else:
                    ws.dy0.zero_()
                    ws.dy1.copy_(dy_carry)
                    # (own kernel: the first use of an ATen op lazily loads its code object - ~60 ms in the middle of training)
                    _lib.call("nlbac_axpby", 1.0, ws.dK[6].data_ptr(), 1.0, dk_carry.data_ptr(), ws.dK[6].numel(),
                              ws.dK[6].data_ptr(), s)
                top_up = ws.dy1           # y1 == stage-6 input
            else:
                tab = TABLEAU[method]
                beta, first_eval = tab["beta"], True
                # out = y0 + h sum c_j K_j
                _lib.call("nlbac_rk_stage_bwd", dout.data_ptr(), None, None, 0, S, fptr(*tab["c_sol"]), h_host,
                          None, 0, P, rpp, ns, ws.dK.data_ptr(), ws.dy0.data_ptr(), 0, None, 0, s)
                top_up = None
            if self.fused:
                self._rk_fused_bwd(ws, u, P, rpp, method, first_eval, need_dy0, need_params, h_host, h_dev, h_stride,
                                   top_up, du, last)
                dy_carry = ws.dy0
                dk_carry = ws.dK[0]
                continue
            for st in range(S - 1, -1, -1):
                if st == 0 and not first_eval:
                    break                  # FSAL alias of the previous step's last stage
                need_dx = (st > 0) or need_dy0
                up = top_up if (st == S - 1 and top_up is not None) else None
                coef = beta[st - 1] if st > 0 else []
                self._stage_backward(ws, st, need_dx, need_params, du, up, coef, h_host, h_dev, h_stride)
            dy_carry = ws.dy0
            dk_carry = ws.dK[0]
        dy0 = steps[0]["ws"].dy0 if need_dy0 else None
        return du, dy0

    def _stage_backward(self, ws, st, need_dx, need_params, du, up, coef, h_host, h_dev, h_stride):
        """Un-fused backward of one stage of the control-affine field: affine_bwd -> mlp_bwd_data[f,g] ->
        rk_stage_bwd (kept as the cross-check of nlbac_node_rk_bwd)."""
        ctx = self.ctx
        P, rpp, n, u = ctx["P"], ctx["rpp"], ctx["n"], ctx["u"]
        ns, nu, S = self.n_s, self.n_u, ws.S
        s = stream_ptr()
        _lib.call("nlbac_affine_combine_bwd", ws.dK[st].data_ptr(), ws.gout[st].data_ptr(), u.data_ptr(),
                  ns, nu, n, 1.0, ws.dG[st].data_ptr() if (need_dx or need_params) else None,
                  du.data_ptr() if du is not None else None, 1, s)
        if need_dx or need_params:
            key = (st, need_params, need_dx)
            io = ws.io_bwd.get(key)
            if io is None:
                io = ws.io_bwd[key] = io_array(2)
                f, g = self.f, self.g
                for i, (net, dy, ld, acts, dz, dx) in enumerate((
                        (f, ws.dK[st], ns, ws.acts_f, ws.dz_f, ws.dXf),
                        (g, ws.dG[st], ns * nu, ws.acts_g, ws.dz_g, ws.dXg))):
                    io[i].dy, io[i].dy_ld = dy.data_ptr(), ld
                    io[i].acts = acts[:, st * ws.n:].data_ptr()
                    io[i].acts_ls = S * ws.n * net.hid
                    if need_params:
                        io[i].dz = dz[:, st * ws.n:].data_ptr()
                    if need_dx:
                        io[i].dx, io[i].dx_ld = dx.data_ptr(), net.in_dim
            _lib.call("nlbac_mlp_bwd_data", self._nets(), io, 2, n, s)
        if need_dx:
            _lib.call("nlbac_rk_stage_bwd", up.data_ptr() if up is not None else None, ws.dXf.data_ptr(),
                      ws.dXg.data_ptr(), self.f.in_dim, st, fptr(*coef) if coef else None, h_host, h_dev,
                      h_stride, P, rpp, ns, ws.dK.data_ptr(), ws.dy0.data_ptr(), 1, None, 0, s)

    def accumulate_param_grads(self, arena, slabs_per_step):
        """dW/db of f_net and g_net over every evaluated stage of every accepted
        step; step i writes slabs [i*slabs_per_step, (i+1)*slabs_per_step).
        Returns the number of slabs written."""
        ctx = self.ctx
        s = stream_ptr()
        if self.adjoint:       # the adjoint solve has integrated the parameter adjoint already: one finished vector
            par = ctx["adj_par"]
            # (under data parallelism the stage derivatives were summed over the ranks already: every rank holds the
            # global vector and hands 1 / world of it to the gradient all-reduce that follows)
            world = self.comm.world if self.comm is not None else 1
            _lib.call("nlbac_axpby", 1.0 / world, par["grad"].data_ptr(), 0.0, None, arena.n, arena.grad.data_ptr(), s)
            return 1
        n_used = 0
        for si, step in enumerate(ctx["steps"]):
            ws = step["ws"]
            S, n = ws.S, ws.n
            st0 = 0 if step["first"] or ctx["method"] != "dopri5" else 1
            rows = (S - st0) * n
            io = io_array(2)
            for i, (net, x, dy, ld, acts, dz) in enumerate((
                    (self.f, ws.Y, ws.dK, self.n_s, ws.acts_f, ws.dz_f),
                    (self.g, ws.Y, ws.dG, self.n_s * self.n_u, ws.acts_g, ws.dz_g))):
                io[i].x0, io[i].x0_dim, io[i].x0_ld = x[st0:].data_ptr(), self.n_s, self.n_s
                io[i].dy, io[i].dy_ld = dy[st0:].data_ptr(), ld
                io[i].acts = acts[:, st0 * n:].data_ptr()
                io[i].dz = dz[:, st0 * n:].data_ptr()
                io[i].acts_ls = S * n * net.hid
            if n_used + slabs_per_step > arena.n_slabs:
                n_used = self._fold_slabs(arena, n_used)
            for i in range(2):
                io[i].grad = arena.grad[n_used:].data_ptr()
            bwd_weights(self._nets(), io, 2, rows, slabs_per_step, arena.n, self.device)
            n_used += slabs_per_step
        return n_used

    def _fold_slabs(self, arena, n_used):
        """A solve with more accepted steps than the arena has gradient slabs: sum what has been written into slab 0,
        clear the rest (the skinny-layer gradients of a step sit in its first slab only) and carry on behind it — the
        one place where the order of the final slab sum differs from one slab set per step."""
        if arena.n_slabs < 2:
            raise _lib.NlbacError("arena has too few gradient slabs (%d) for this solve" % arena.n_slabs)
        tmp = self._buf("grad_fold", arena.n)
        s = stream_ptr()
        _lib.call("nlbac_reduce_slabs", tmp.data_ptr(), arena.grad.data_ptr(), n_used, arena.n, arena.n, s)
        _lib.call("nlbac_axpby", 1.0, tmp.data_ptr(), 0.0, None, arena.n, arena.grad.data_ptr(), s)
        _lib.call("nlbac_fill", arena.grad[1:].data_ptr(), 0.0, (arena.n_slabs - 1) * arena.n, s)
        return 1


# ---------------------------------------------------------------------------
# Non-affine field  dx/dt = net([x, c])  with carried inputs c = (u, t, ...) constant over the step
# (SimulatedCars: C/sac_cbf_clf/model.py:179-205).  Same RK machinery, stage by stage on nlbac_mlp_*.
# ---------------------------------------------------------------------------

class ConcatNodeSolver(ConcatAdjoint, AffineNodeSolver):
    """``u`` here is the (n, n_carry) block of carried inputs; ``backward`` returns its gradient."""
    STEP_WS = _ConcatStepWS
    OUT_MAP_IN_RK = False      # the single-net kernels evaluate no out-map

    def __init__(self, node, device):
        self.node, self.net = node, node.net_handle
        self.f = self.g = self.net            # (base-class bookkeeping only)
        self.n_s, self.n_u = node.n_s, node.n_carry
        # one nlbac_concat_rk_fwd / _bwd launch per RK step (nets of <= 128 hidden units; wider ones run stage by stage)
        self.fused = self.net.hid <= 128
        self._init_state(device)
        # input normalisation / output de-normalisation lives inside the fused step kernels only
        self.norm = node.norm_device() if getattr(node, "normalized", False) else None
        if self.norm is not None and not self.fused:
            raise _lib.NlbacError("a normalised NODE needs the fused step kernels (hidden width <= 128)")

    def _nets(self):
        if self._net_arr is None:
            self._net_arr = mlp_array([self.net.desc])
        return self._net_arr

    def _interp_nets(self):
        return C.byref(self.net.desc), None

    def _fit_words_on(self):
        return False

    def _rk_fused(self, ws, y0, u, P, rpp, method, st0, st1, h_host=None, h_dev=None, c_out=None, out=None,
                  c_err=None, err=None, save_acts=True, chain=None):
        beta, S = self._beta(method)
        save_acts = save_acts and not self.adjoint       # (the adjoint re-computes every stage it differentiates)
        _lib.call("nlbac_concat_rk_fwd", C.byref(self.net.desc), y0.data_ptr(), u.data_ptr(), P, rpp, st0, st1, S, beta,
                  c_out, len(c_out) if c_out is not None else 0, c_err, len(c_err) if c_err is not None else 0,
                  fptr(*h_host) if h_host is not None else None, h_dev, _lib.DOPRI_CTL if h_dev else 0,
                  ws.K.data_ptr(), ws.Y.data_ptr(), ws.acts.data_ptr() if save_acts else None,
                  ws.S * P * rpp * ws.wa, 1 if (ws.bits and (save_acts or not self.rows_sums)) else 0,
                  out.data_ptr() if out is not None else None,
                  err.data_ptr() if err is not None else None,
                  self.norm.data_ptr() if self.norm is not None else None,
                  ws.Xn.data_ptr() if (self.norm is not None and save_acts and self.keep_acts) else None,
                  C.byref(chain) if chain is not None else None, stream_ptr())
        self.nfe += st1 - st0

    def _rk_fused_bwd(self, ws, u, P, rpp, method, first_eval, need_dy0, need_params, h_host, h_dev, h_stride, top_up,
                      du, last, chain=None, back_idx=0):
        beta_arr, _ = self._beta(method)
        S = ws.S
        _lib.call("nlbac_concat_rk_bwd", C.byref(self.net.desc), P, rpp, S, 0 if first_eval else 1, S,
                  1 if need_dy0 else 0, beta_arr, h_host, h_dev, h_stride, ws.acts.data_ptr(),
                  S * ws.n * ws.wa, 1 if ws.bits else 0, ws.dz.data_ptr() if need_params else None, ws.dK.data_ptr(),
                  top_up.data_ptr() if top_up is not None else None, ws.dy0.data_ptr(), 1,
                  du.data_ptr() if du is not None else None, 0 if last else 1,
                  self.norm.data_ptr() if self.norm is not None else None,
                  ws.dyn.data_ptr() if (self.norm is not None and need_params) else None,
                  C.byref(chain) if chain is not None else None, back_idx, stream_ptr())

    def _eval_io(self, x, k_out, c, acts=None, ls=0):
        io = io_array(1)
        io[0].x0, io[0].x0_dim, io[0].x0_ld = x.data_ptr(), self.n_s, self.n_s
        io[0].x1, io[0].x1_dim, io[0].x1_ld = c.data_ptr(), self.n_u, self.n_u
        io[0].y, io[0].y_ld = k_out.data_ptr(), self.n_s
        if acts is not None:
            io[0].acts, io[0].acts_ls = acts.data_ptr(), ls
        return io

    def _eval(self, x, u, n, k_out, g_out, io=None):
        if io is None:
            io = self._eval_io(x, k_out, u)
        _lib.call("nlbac_mlp_fwd", self._nets(), io, 1, n, stream_ptr())
        self.nfe += 1

    def _probe_eval(self, ytmp, u, n, ktmp, gtmp):
        self._eval(ytmp, u, n, ktmp, None)

    def _stage_eval(self, ws, st, u):
        n, S = ws.n, ws.S
        io = ws.io_fwd.get(st)
        if io is None:
            io = ws.io_fwd[st] = self._eval_io(ws.Y[st], ws.K[st], u, ws.acts[:, st * n:], S * n * self.net.hid)
        io[0].x1 = u.data_ptr()      # (the cached descriptor outlives a solve; the carried inputs are the caller's tensor)
        self._eval(ws.Y[st], u, n, ws.K[st], None, io)

    def _stage_backward(self, ws, st, need_dx, need_params, du, up, coef, h_host, h_dev, h_stride):
        ctx = self.ctx
        P, rpp, n = ctx["P"], ctx["rpp"], ctx["n"]
        ns, S, net = self.n_s, ws.S, self.net
        s = stream_ptr()
        key = (st, need_params)
        io = ws.io_bwd.get(key)
        if io is None:
            io = ws.io_bwd[key] = io_array(1)
            io[0].dy, io[0].dy_ld = ws.dK[st].data_ptr(), ns
            io[0].acts, io[0].acts_ls = ws.acts[:, st * n:].data_ptr(), S * n * net.hid
            if need_params:
                io[0].dz = ws.dz[:, st * n:].data_ptr()
            io[0].dx, io[0].dx_ld = ws.dX.data_ptr(), net.in_dim
        _lib.call("nlbac_mlp_bwd_data", self._nets(), io, 1, n, s)
        # dY = [up] + dX[:, :n_s] ; dy0 += dY ; dK[j] += beta h dY ; d carried += dX[:, n_s:]
        _lib.call("nlbac_rk_stage_bwd", up.data_ptr() if up is not None else None, ws.dX.data_ptr(), None,
                  net.in_dim, st, fptr(*coef) if coef else None, h_host, h_dev, h_stride, P, rpp, ns,
                  ws.dK.data_ptr(), ws.dy0.data_ptr(), 1, du.data_ptr() if du is not None else None, self.n_u, s)

    def accumulate_param_grads(self, arena, slabs_per_step):
        ctx = self.ctx
        if self.adjoint:       # the adjoint solve has integrated the parameter adjoint already (see the base class)
            return AffineNodeSolver.accumulate_param_grads(self, arena, slabs_per_step)
        n_used = 0
        for si, step in enumerate(ctx["steps"]):
            ws = step["ws"]
            S, n = ws.S, ws.n
            st0 = 0 if step["first"] or ctx["method"] != "dopri5" else 1
            rows = (S - st0) * n
            io = io_array(1)
            if self.norm is not None:      # the net saw normalised inputs and its output is scaled: use what the kernels kept
                io[0].x0, io[0].x0_dim, io[0].x0_ld = ws.Xn[st0:].data_ptr(), self.net.in_dim, self.net.in_dim
                io[0].dy, io[0].dy_ld = ws.dyn[st0:].data_ptr(), self.n_s
            else:
                ws.c_rep.view(S, n, self.n_u).copy_(ctx["u"].unsqueeze(0).expand(S, n, self.n_u))
                io[0].x0, io[0].x0_dim, io[0].x0_ld = ws.Y[st0:].data_ptr(), self.n_s, self.n_s
                io[0].x1, io[0].x1_dim, io[0].x1_ld = ws.c_rep[st0 * n:].data_ptr(), self.n_u, self.n_u
                io[0].dy, io[0].dy_ld = ws.dK[st0:].data_ptr(), self.n_s
            io[0].acts = ws.acts[:, st0 * n:].data_ptr()
            io[0].dz = ws.dz[:, st0 * n:].data_ptr()
            io[0].acts_ls = S * n * self.net.hid
            if n_used + slabs_per_step > arena.n_slabs:
                n_used = self._fold_slabs(arena, n_used)
            io[0].grad = arena.grad[n_used:].data_ptr()
            bwd_weights(self._nets(), io, 1, rows, slabs_per_step, arena.n, self.device)
            n_used += slabs_per_step
        return n_used


# ---------------------------------------------------------------------------
# torchdiffeq-shaped entry (SURVEY.md §8b "Solver entry"): the call the reference makes at
# U/sac_cbf_clf/sac_cbf_clf.py:453,577 and U/sac_cbf_clf/model.py:252 —
#     odeint(model, cat(state, action), tensor([0, dt]), method=..., atol=1e-7, rtol=1e-5)[-1][:, :n_s]
# — on the device kernels, differentiable w.r.t. y0 and the model's parameters through torch.autograd.
# The agent itself drives the solvers directly (no autograd graph); this entry is for reference-shaped code.
# ---------------------------------------------------------------------------
def _solver_of(func, adjoint=False):
    """The (cached) solver of a ``NeuralODEModel`` of this build; a model that is not part of an agent gets its own
    parameter arena on the current device.  The adjoint entry keeps a solver of its own (it saves nothing in forward)."""
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.odeint integrates this build's NeuralODEModel (its field runs as HIP kernels); "
                        "got %s" % type(func).__name__)
    key = "_odeint_solver_adj" if adjoint else "_odeint_solver"
    sv = getattr(func, key, None)
    if sv is None:
        handles = func.device_handles()
        sv = (AffineNodeSolver if func.affine else ConcatNodeSolver)(func, handles[0].arena.device)
        sv.keep_acts = True                  # parameter gradients need the pre-activation gradients of every stage
        sv.adjoint = bool(adjoint)
        setattr(func, key, sv)
    return sv


class _OdeintSolve(PackedSolve):
    """``odeint`` / ``odeint_adjoint`` over [t0, t0 + dt] as ``ode_node.SolveNode``'s solve: what is kept is the cached
    solver, which holds one solve's state.  ``adjoint``: False, or "params" / "no-params" (``adjoint_params=()``)."""
    api = "odeint"

    def __init__(self, func, method, dt, atol, rtol, adjoint):
        PackedSolve.__init__(self, func)
        self.args, self.adjoint, self.with_params = (method, dt, atol, rtol), bool(adjoint), adjoint != "no-params"

    def forward(self, y0):
        sv = self.kept = _solver_of(self.func, self.adjoint)
        ns, nu = sv.n_s, sv.n_u
        assert y0.dim() == 2 and y0.shape[1] == ns + nu, "y0 must be (batch, %d)" % (ns + nu)
        y0, x0, u = self.split(y0.float())
        x1 = sv.forward(x0, u, 1, y0.shape[0], *self.args)
        self.solve_id = sv.stats["solves"]
        return torch.stack([y0, torch.cat([x1, u], dim=1)])

    def backward(self, g, need_in, need_p):
        sv, ns = self.kept, self.ns
        assert sv.stats["solves"] == self.solve_id, \
            "odeint: backward must run before the next solve with the same model (the solver keeps one solve's state)"
        du, dy0 = sv.backward(g[1][:, :ns].contiguous(), need_du=True, need_params=need_p, need_dy0=True)
        gy0 = self.grad_y0(g, dy0, du, g[1][:, ns:], self) if need_in[0] else None
        if not need_p:
            return gy0, None
        arena = self.func.device_handles()[0].arena
        n_steps = max(1, len(sv.ctx.get("steps") or [None]))
        return gy0, _reduce(arena, sv.accumulate_param_grads(arena, max(1, arena.n_slabs // n_steps)))


def _odeint(func, y0, t, method, atol, rtol, adjoint, options):
    # the one option served: options=dict(step_size=s) under euler / rk4 (ode_grid.odeint_grid's step_size)
    sub = options.pop("options", None)
    if options:
        raise TypeError("odeint: unsupported options %s" % sorted(options))
    if sub is not None:
        if not isinstance(sub, dict) or set(sub) - {"step_size"}:
            raise TypeError("odeint: unsupported options %s" % (sorted(sub, key=str) if isinstance(sub, dict) else type(sub).__name__))
        if sub.get("step_size") is not None:
            if adjoint:
                raise NotImplementedError("odeint_adjoint: step_size is not offered (the adjoint solve steps once over "
                                          "[t0, t1]); use odeint, or rollout / odeint_grid with adjoint=True and step_size")
            if method == "dopri5":
                raise ValueError("odeint: step_size goes with method='euler' or 'rk4'; torchdiffeq's dopri5 ignores it, "
                                 "which this build does not do silently")
            if torch.as_tensor(t).numel() > 2:
                raise NotImplementedError("odeint: the reference only ever integrates over t = [0, dt]; got %d time "
                                          "points (ode_grid.odeint_grid takes a longer grid)" % torch.as_tensor(t).numel())
            from .ode_grid import odeint_grid
            return odeint_grid(func, y0, t, method=method, step_size=sub["step_size"])
    from .sac_cbf_clf.model import NeuralODEModel
    if not isinstance(func, NeuralODEModel):
        raise TypeError("nlbac_amd.odeint integrates this build's NeuralODEModel (its field runs as HIP kernels); "
                        "got %s" % type(func).__name__)
    t = torch.as_tensor(t)
    if t.numel() != 2:
        raise NotImplementedError("odeint: the reference only ever integrates over t = [0, dt]; got %d time points "
                                  "(ode_grid.odeint_grid takes a longer grid, with adjoint=True the continuous adjoint on it; "
                                  "ode_dense.odeint_dense reads one dopri5 solve at every point of one, "
                                  "ode_dense.odeint_dense_adjoint with the continuous adjoint as its backward)"
                                  % t.numel())
    dt = float(t[1]) - float(t[0])
    func.refresh_device_weights()
    return SolveNode.apply(_OdeintSolve(func, method, dt, float(atol), float(rtol), adjoint), 1, y0, *func.parameters())


def odeint(func, y0, t, *, method="dopri5", atol=1e-7, rtol=1e-5, **options):
    """``torchdiffeq.odeint`` for this build's NODE models on ``t = [t0, t1]``: returns ``stack([y0, y(t1)])`` with the
    carried control columns passed through, differentiable w.r.t. ``y0`` and ``func.parameters()``.  ``method`` is
    ``'euler'`` / ``'rk4'`` (one step over the interval, torchdiffeq's fixed-grid semantics; with
    ``options=dict(step_size=s)`` steps of ``s``, the last one cut at ``t1``: ``ode_grid.odeint_grid``'s ``step_size``)
    or ``'dopri5'`` (which refuses ``step_size``; no other option is served).
    The packed MFMA copies of the weights are refreshed first, so a ``torch.optim`` step on ``func.parameters()``
    between calls is picked up.  For several intervals ahead with a new control each, differentiated as a whole, use
    ``nlbac_amd.rollout.rollout``; for the solution at every point of a longer time grid, use
    ``nlbac_amd.ode_grid.odeint_grid`` (euler / rk4) or ``nlbac_amd.ode_dense.odeint_dense`` (one dopri5 solve)."""
    return _odeint(func, y0, t, method, atol, rtol, False, options)


def odeint_adjoint(func, y0, t, *, method="dopri5", atol=1e-7, rtol=1e-5, adjoint_params=None, **options):
    """``torchdiffeq.odeint_adjoint`` (0.2.3) on ``t = [t0, t1]``: the same forward solve, keeping only y(t1); the
    backward integrates the augmented state [y, adj_y, adj_params] from t1 to t0 with the same method and tolerances
    (``adjoint_rtol`` / ``adjoint_atol`` / ``adjoint_method`` default to the forward's in torchdiffeq; only those
    defaults are offered) under torchdiffeq's default mixed adjoint norm.  Memory does not grow with the number of
    steps, and the gradient equals direct back-propagation only to solver tolerance.  ``adjoint_params``: ``None`` —
    every parameter of ``func`` (torchdiffeq's default, ``find_parameters``); ``()`` — no parameter adjoint (it then
    also stays out of the step-size norm).  The reference never calls this; semantics follow the
    published algorithm.  On a time grid (more than two points, dopri5) the same call is
    ``nlbac_amd.ode_dense.odeint_dense_adjoint``: one dense forward solve, the adjoint walked over the grid's intervals."""
    if adjoint_params is not None and len(tuple(adjoint_params)) != 0:
        raise NotImplementedError("odeint_adjoint: adjoint_params is None (all of func's parameters) or ()")
    return _odeint(func, y0, t, method, atol, rtol, "no-params" if adjoint_params is not None else "params", options)
