"""The continuous adjoint of the NODE solvers (``odeint_adjoint``; ``solver.adjoint = True``): the backward of a
solve as a second solve, with nothing of the forward kept.  ``AffineAdjoint`` / ``ConcatAdjoint`` are the adjoint halves
of ``odeint.AffineNodeSolver`` / ``odeint.ConcatNodeSolver``; they use the solver's scratch buffers (``_buf``), its
control-block reader (``ctl``), its tableau coefficients (``_beta``, ``_coef``) and the solve's ``ctx``."""
import ctypes as C

import torch

from . import _lib
from ._lib import fptr
from .arena import bwd_weights, io_array, stream_ptr
from .ode_consts import CTL_DONE, CTL_H0, CTL_HUSED, CTL_NSTEPS, CTL_RATIO, TABLEAU, ctl_field_ptr


class AffineAdjoint:
    """Continuous adjoint of the control-affine field ``dx/dt = f(x) + g(x) u``."""
    # torchdiffeq 0.2.3 OdeintAdjointMethod.backward restated on the device: the augmented state z = [y | a_x | a_u]
    # (+ the parameter adjoint, a quadrature) is integrated from t1 back to t0 with the forward's method and
    # tolerances and the mixed default adjoint norm; one nlbac_node_adj_step launch per RK step re-computes the nets on
    # every stage input and back-propagates a_x through them, so nothing of the forward solve is kept.  The dopri5
    # attempts are a device-driven chain (kernels skip problems whose solve is done, an accepted step is handed over
    # by nlbac_adj_commit); the host looks at the control block once per chain, not once per attempt.
    ADJ_MAX_ATTEMPTS = 1000

    def _init_adjoint(self):
        self._adj_ip_ok = None     # nlbac_node_adj_interp_ok of the nets, asked once (``_adj_interp_fold``)
        self._adj_chain = 1        # attempts the last dopri5 adjoint solve needed = launches enqueued before the first read
        self._adj_par_cur = None   # the parameter adjoint of the backward in progress (``_adj_params_begin``)

    def _adj_ws(self, n, S):
        key = ("adj", n, S)
        pool = self._scratch.setdefault(n, {})
        w = pool.get(key)
        if w is None:
            W = 2 * self.n_s + self.n_u
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
            w = pool[key] = dict(Z0=z(n, W), Z1=z(n, W), KZ=z(S, n, W), ERR=z(n, W), OUT=z(n, W), W=W)
        return w

    def _adj_interp_fold(self):
        """The attempt launches of the adjoint solve write the interpolant of z at t_end themselves (no
        nlbac_dopri_interp_fwd launch behind the solve) where the kernel that serves the nets does so."""
        ok = self._adj_ip_ok
        if ok is None:
            ok = self._adj_ip_ok = bool(_lib.load().nlbac_node_adj_interp_ok(C.byref(self.f.desc), C.byref(self.g.desc)))
        return ok and self.interp_fold

    def _adj_step(self, w, u, P, rpp, method, st0, st1, h_host=None, h_dev=None, ctl=None, c_out=None, c_err=None,
                  keep=None, interp=False):
        beta, S = self._beta(method)
        f, g = self.f, self.g
        k = keep or {}
        dp = lambda t: t.data_ptr() if t is not None else None
        _lib.call("nlbac_node_adj_step", C.byref(f.desc), C.byref(g.desc), u.data_ptr(), P, rpp, st0, st1, S, beta,
                  c_out, len(c_out) if c_out is not None else 0, c_err, len(c_err) if c_err is not None else 0,
                  fptr(*h_host) if h_host is not None else None, h_dev, _lib.DOPRI_CTL if h_dev else 0, ctl,
                  w["Z0"].data_ptr(), w["KZ"].data_ptr(), w["Z1"].data_ptr() if c_out is not None else None,
                  w["ERR"].data_ptr() if c_err is not None else None, dp(k.get("ZS")), dp(k.get("dG")),
                  dp(k.get("acts_f")), k.get("ls_f", 0), dp(k.get("acts_g")), k.get("ls_g", 0), dp(k.get("dz_f")),
                  dp(k.get("dz_g")), w["OUT"].data_ptr() if interp else None, self.ctx["t_end"], stream_ptr())
        self.nfe += st1 - st0
        if keep:
            for st in range(st0, st1):
                self._adj_stage_dw(self._adj_par_cur, st)

    def _adj_norm_control(self, a, b, w, u, mode, P, rpp, ctl, pnorm=None):
        ctx = self.ctx
        ns, nu, s = self.n_s, self.n_u, stream_ptr()
        nblk = (rpp + 255) // 256
        part = self._buf("adj_part", P, nblk, 4)
        dp = lambda t: t.data_ptr() if t is not None else None
        if self.comm is not None and self.comm.world > 1:
            _lib.call("nlbac_adj_norm_control", dp(a), dp(b), w["Z0"].data_ptr(), w["Z1"].data_ptr(), dp(u), mode,
                      ctx["rtol"], ctx["atol"], ns, nu, rpp, P, ctx["t_end"], None, part.data_ptr(), None,
                      ctl.data_ptr(), None, 0.0, s)
            sums = self._buf("adj_psum", P, 1, 4)
            for p in range(P):
                _lib.call("nlbac_sum_partials", part[p].data_ptr(), nblk, 4, 1.0, sums[p].data_ptr(), s)
            self.comm.all_reduce_(sums)
            _lib.call("nlbac_adj_control", sums.data_ptr(), 1, mode, ns, nu, rpp * self.comm.world, P, ctx["t_end"],
                      dp(pnorm), ctl.data_ptr(), s)
            return
        tickets = self._buf("adj_tickets", P, dtype=torch.int32)
        # (an attempt's controller leaves the host's copy of the control block in pinned memory itself: no copy launch
        #  between the decision and the host; see ControlBlockReader.posted)
        host, seq = None, 0.0
        if mode == 2 and not torch.cuda.is_current_stream_capturing():
            host = self.ctl.io(P)[1].data_ptr()
            seq = self.ctl.next_stamp(ctx)
        ctx["adj_ctl_host"] = host is not None
        _lib.call("nlbac_adj_norm_control", dp(a), dp(b), w["Z0"].data_ptr(), w["Z1"].data_ptr(), dp(u), mode,
                  ctx["rtol"], ctx["atol"], ns, nu, rpp, P, ctx["t_end"], dp(pnorm), part.data_ptr(),
                  tickets.data_ptr(), ctl.data_ptr(), host, seq, s)

    # -- parameter adjoint (a quadrature beside the per-row state; single-problem solves) -----------------
    ADJ_SUB_SLABS = 40       # row slabs of one stage's weight-gradient GEMM (workgroups: layers x slabs x nets)

    def _adj_params_begin(self, w, n, S):
        ctx = self.ctx
        assert ctx["P"] == 1, "parameter gradients are only taken on single-problem solves"
        key = ("adj_par", n, S)
        pool = self._scratch.setdefault(n, {})
        par = pool.get(key)
        if par is None:
            dev = self.device
            z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
            arena = self.f.arena
            NP = arena.n
            keep = self._adj_keep(z, w, n, S)
            segs = [(arena.offset_of[id(p)], p.numel()) for p in self.node.parameters()]
            par = pool[key] = dict(
                keep=keep, NP=NP, K=z(S, NP), th0=z(NP), th1=z(NP), out=z(NP), slabs=z(self.ADJ_SUB_SLABS, NP),
                seg_off=torch.tensor([o for o, _ in segs], dtype=torch.int32, device=dev),
                seg_len=torch.tensor([l for _, l in segs], dtype=torch.int32, device=dev), n_seg=len(segs),
                pseg=z(2 * len(segs)), ticket=z(1, dtype=torch.int32), pnorm=z(2), io={}, n=n, S=S, w=w)
        _lib.call("nlbac_fill", par["th0"].data_ptr(), 0.0, par["NP"], stream_ptr())
        par["grad"] = None
        return par

    def _adj_keep(self, z, w, n, S):
        """What the step kernel keeps of every stage for the parameter adjoint's quadrature (``_adj_stage_dw``)."""
        f, g, ns, nu = self.f, self.g, self.n_s, self.n_u
        return dict(ZS=z(S, n, w["W"]), dG=z(S, n, ns * nu), acts_f=z(f.n_layers - 1, S * n, f.hid),
                    acts_g=z(g.n_layers - 1, S * n, g.hid), dz_f=z(f.n_layers - 1, S * n, f.hid),
                    dz_g=z(g.n_layers - 1, S * n, g.hid), ls_f=S * n * f.hid, ls_g=S * n * g.hid)

    def _adj_stage_dw(self, par, st):
        """K_theta[st] = sum over the rows of stage ``st`` of (dF/dtheta)^T a_x: nlbac_mlp_bwd_weights on what the
        step kernel kept of that stage (row slabs), then the slab sum."""
        k, n, S, w = par["keep"], par["n"], par["S"], par["w"]
        W, ns, nu = w["W"], self.n_s, self.n_u
        io = par["io"].get(st)
        if io is None:
            io = par["io"][st] = io_array(2)
            ZS = k["ZS"][st]
            for i, (net, acts, dz) in enumerate(((self.f, k["acts_f"], k["dz_f"]), (self.g, k["acts_g"], k["dz_g"]))):
                io[i].x0, io[i].x0_dim, io[i].x0_ld = ZS.data_ptr(), ns, W
                io[i].acts, io[i].dz = acts[:, st * n:].data_ptr(), dz[:, st * n:].data_ptr()
                io[i].acts_ls = S * n * net.hid
                io[i].grad = par["slabs"].data_ptr()
            io[0].dy, io[0].dy_ld = ZS.data_ptr() + 4 * ns, W              # cotangent of f_net's output: a_x
            io[1].dy, io[1].dy_ld = k["dG"][st].data_ptr(), ns * nu        # of g_net's: a_x u^T
        bwd_weights(self._nets(), io, 2, n, self.ADJ_SUB_SLABS, par["NP"], self.device)
        _lib.call("nlbac_reduce_slabs", par["K"][st].data_ptr(), par["slabs"].data_ptr(), self.ADJ_SUB_SLABS,
                  par["NP"], par["NP"], stream_ptr())
        if self.comm is not None and self.comm.world > 1:
            # sample-sharded solve: the parameter adjoint is a sum over ALL rows, and its norm takes part in the step
            # control — every rank must form it from the same (global) stage derivative, or the ranks' accept / done
            # decisions part ways and their collectives no longer pair up
            self.comm.all_reduce_(par["K"][st])

    def _adj_params_norm(self, par, mode, cp, h_host=None, c_sol=None):
        ctx = self.ctx
        _lib.call("nlbac_adj_param_norm", mode, par["th0"].data_ptr(), par["K"].data_ptr(), par["NP"], par["S"],
                  c_sol if c_sol is not None else self._coef("sol"), self._coef("err") if c_sol is None else fptr(*([0.0] * par["S"])),
                  fptr(h_host) if h_host is not None else None, cp if h_host is None else None,
                  par["seg_off"].data_ptr(), par["seg_len"].data_ptr(), par["n_seg"], ctx["rtol"], ctx["atol"],
                  cp if (mode == 2 and h_host is None) else None, par["th1"].data_ptr(), par["pseg"].data_ptr(),
                  par["ticket"].data_ptr(), par["pnorm"].data_ptr(), stream_ptr())
        return par["pnorm"]

    def _adj_params_commit(self, par, cp):
        NP = par["NP"]
        _lib.call("nlbac_adj_commit", cp, NP // 4, NP // 4, 4, par["th0"].data_ptr(), par["th1"].data_ptr(),
                  par["K"][0].data_ptr(), par["K"][6].data_ptr(), stream_ptr())

    def _adj_params_finish(self, par, cp):
        NP = par["NP"]
        _lib.call("nlbac_dopri_interp_fwd", par["th0"].data_ptr(), par["th1"].data_ptr(), par["K"].data_ptr(), None,
                  None, cp, 1, NP // 4, 4, par["out"].data_ptr(), 0, None, stream_ptr())
        par["grad"] = par["out"]
        self.ctx["adj_par"] = par

    def _adj_params_fixed(self, par, w, c_sol, h):
        """fixed grid: theta_bar(t0) = h sum_j c_sol[j] K_theta[j]"""
        self._adj_params_norm(par, 2, None, h_host=h, c_sol=fptr(*c_sol))
        par["grad"] = par["th1"]
        self.ctx["adj_par"] = par

    def backward_adjoint(self, dout, need_du=True, need_params=False, need_dy0=False):
        """dL/du, dL/dy0 (and, with ``need_params``, the parameter adjoint for ``accumulate_param_grads``) from
        dL/dy(t1) = ``dout`` by solving the adjoint system backwards from the forward's y(t1)."""
        ctx = self.ctx
        P, rpp, n, u, method = ctx["P"], ctx["rpp"], ctx["n"], ctx["u"], ctx["method"]
        ns, nu, s = self.n_s, self.n_u, stream_ptr()
        assert dout.shape == (n, ns) and dout.is_contiguous()
        self._cur_n = n
        S = 7 if method == "dopri5" else len(TABLEAU[method]["c_sol"])
        w = self._adj_ws(n, S)
        par = self._adj_par_cur = self._adj_params_begin(w, n, S) if need_params else None
        _lib.call("nlbac_adj_pack", ctx["out"].data_ptr(), dout.data_ptr(), ns, nu, n, w["Z0"].data_ptr(), s)
        if method in ("euler", "rk4"):
            tab = TABLEAU[method]
            h = [ctx["t_end"]] * P
            self._adj_step(w, u, P, rpp, method, 0, S, h_host=h, c_out=fptr(*tab["c_sol"]),
                           keep=par and par["keep"])
            if par:
                self._adj_params_fixed(par, w, tab["c_sol"], h[0])
            res = w["Z1"]
            ctx["adjoint_info"] = None
        else:
            res = self._adj_dopri(w, u, P, rpp, par)
        du = self._buf("du", n, nu) if need_du else None
        dy0 = self._buf("dy0_adj", n, ns) if need_dy0 else None
        if du is not None or dy0 is not None:
            _lib.call("nlbac_adj_unpack", res.data_ptr(), ns, nu, n, dy0.data_ptr() if dy0 is not None else None,
                      du.data_ptr() if du is not None else None, s)
        return du, dy0

    # -- the adjoint of a dense dopri5 solve (ode_dense.odeint_dense_adjoint) -----------------------------------------------
    def backward_adjoint_dense(self, out, dout, c, lengths, need_params):
        """torchdiffeq 0.2.3 ``OdeintAdjointMethod.backward`` on a time grid, after this solver's dense forward: ``out`` /
        ``dout`` (T, n, n_s + n_c) contiguous — the stored outputs and their gradient, read in place — ``c`` (n, n_c) the
        carried columns, ``lengths[j - 1]`` the length of [t[j-1], t[j]].  The intervals are solved last to first, each a
        fresh adaptive solve over [0, length] (``_adj_dopri``: its own f0, Hairer step, probe and attempts).  At an
        interval's upper end nlbac_adj_dense_restart RESETS the state part of z to the stored ``out[j]`` and adds
        ``dout[j]``'s state columns to a_x; a_x, a_c and the parameter adjoint are CARRIED from the interval above (the
        parameter adjoint by a buffer swap: what the interpolation at the lower end wrote is the next interval's th0) and
        take part in the mixed norm.  ``dout``'s carried columns stay out of the solve: the caller adds them.
        Returns (a_x, a_c) at t[0] in the solver's buffers and the parameter adjoint (``par["out"]``) or None;
        ``ctx["adjoint_info"]`` lists what ``_adj_dopri`` records per interval, last interval first.  One host wait on the
        control block per chain of attempts, so at least one per interval."""
        ctx = self.ctx
        n, ns, nu, s = ctx["n"], self.n_s, self.n_u, stream_ptr()
        if self.comm is not None and self.comm.world > 1:
            raise NotImplementedError("odeint_dense_adjoint: not offered on a sample-sharded solve (comm.world = %d)"
                                      % self.comm.world)
        assert ctx["P"] == 1 and ctx["method"] == "dopri5", "the dense adjoint follows a single-problem dopri5 solve"
        ld = ns + nu
        for t in (out, dout):
            assert t.shape == (len(lengths) + 1, n, ld) and t.is_contiguous() and t.dtype == torch.float32
        assert c.shape == (n, nu) and c.is_contiguous()
        self._cur_n = n
        w = self._adj_ws(n, 7)
        par = self._adj_par_cur = self._adj_params_begin(w, n, 7) if need_params else None
        infos, prev = [], None
        for j in range(len(lengths), 0, -1):
            ctx["t_end"] = lengths[j - 1]
            _lib.call("nlbac_adj_dense_restart", out[j].data_ptr(), ld, dout[j].data_ptr(), ld, prev, ns, nu, n,
                      w["Z0"].data_ptr(), s)
            if par and prev is not None:
                par["th0"], par["out"] = par["out"], par["th0"]
            prev = self._adj_dopri(w, c, 1, n, par).data_ptr()
            infos.append(ctx["adjoint_info"])
        ctx["adjoint_info"] = infos
        a_x, a_c = self._buf("dy0_adj", n, ns), self._buf("du", n, nu)
        _lib.call("nlbac_adj_unpack", prev, ns, nu, n, a_x.data_ptr(), a_c.data_ptr(), s)
        return a_x, a_c, (par["out"] if par else None)

    # -- an output interval solved backwards in fine steps (rollout / odeint_grid with adjoint=True and step_size, chained) --
    def adjoint_grid_begin(self, n, method, need_params, atol=1e-7, rtol=1e-5):
        """Start a chained grid adjoint on ``n`` rows (``ode_traj.ChainSubAdjoint``): a solve state of its own — no
        forward of this solver precedes it — and, with ``need_params``, the zeroed parameter adjoint."""
        self._touch(n)
        self.ctx = dict(P=1, rpp=n, n=n, method=method, t_end=0.0, atol=atol, rtol=rtol)
        S = len(TABLEAU[method]["c_sol"])
        w = self._adj_ws(n, S)
        self._adj_par_cur = self._adj_params_begin(w, n, S) if need_params else None
        return self._adj_par_cur

    def adjoint_interval(self, y_end, a_end, u, method, hs, par):
        """One output interval: z = [``y_end`` | ``a_end`` | 0] at its upper end carried through the fine steps ``hs``
        (applied in that order, from the upper end down) — one nlbac_*_adj_step launch per fine step, Z0 <-> Z1 swapped
        in between, no reset inside; with ``par`` the parameter adjoint goes on accumulating, th1 = th0 + h sum c_sol[j]
        K_theta[j] (nlbac_adj_param_norm mode 2), th0 <-> th1 swapped likewise.  Returns (du, dy0) in the solver's buffers."""
        n, ns, nu, s = self.ctx["n"], self.n_s, self.n_u, stream_ptr()
        tab = TABLEAU[method]
        S, c_sol = len(tab["c_sol"]), fptr(*tab["c_sol"])
        w = self._adj_ws(n, S)
        _lib.call("nlbac_adj_pack", y_end.data_ptr(), a_end.data_ptr(), ns, nu, n, w["Z0"].data_ptr(), s)
        for h in hs:
            self._adj_step(w, u, 1, n, method, 0, S, h_host=[h], c_out=c_sol, keep=par and par["keep"])
            w["Z0"], w["Z1"] = w["Z1"], w["Z0"]
            if par:
                self._adj_params_norm(par, 2, None, h_host=h, c_sol=c_sol)
                par["th0"], par["th1"] = par["th1"], par["th0"]
        du, dy0 = self._buf("du", n, nu), self._buf("dy0_adj", n, ns)
        _lib.call("nlbac_adj_unpack", w["Z0"].data_ptr(), ns, nu, n, dy0.data_ptr(), du.data_ptr(), s)
        return du, dy0

    def _adj_dopri(self, w, u, P, rpp, par):
        ctx = self.ctx
        n, S, s = ctx["n"], 7, stream_ptr()
        ctl = self._buf("adj_ctl", P, _lib.DOPRI_CTL, dtype=torch.float64)
        cp = ctl.data_ptr()
        KZ = w["KZ"]
        keep = par and par["keep"]
        self.ctl.begin(ctx)           # (the adjoint solve's own range of stamps)
        # f0 = G(z(t1)) and Hairer's initial step
        self._adj_step(w, u, P, rpp, "dopri5", 0, 1, h_host=[0.0] * P, keep=keep)
        pn = self._adj_params_norm(par, 0, cp) if par else None
        self._adj_norm_control(KZ[0], None, w, u, 0, P, rpp, ctl, pn)
        self._adj_step(w, u, P, rpp, "probe", 1, 2, h_dev=ctl_field_ptr(cp, CTL_H0), keep=keep)
        pn = self._adj_params_norm(par, 1, cp) if par else None
        self._adj_norm_control(KZ[1], KZ[0], w, None, 1, P, rpp, ctl, pn)
        c_sol, c_err = self._coef("sol"), self._coef("err")
        chain = max(1, int(self._adj_chain))
        attempts = 0
        ip = self._adj_interp_fold()
        while True:
            for i in range(chain):
                if attempts:
                    # accepted and not finished: z0 <- z1, first stage <- last stage (FSAL); decided on the device
                    _lib.call("nlbac_adj_commit", cp, rpp, n, w["W"], w["Z0"].data_ptr(), w["Z1"].data_ptr(),
                              KZ[0].data_ptr(), KZ[6].data_ptr(), s)
                    if par:
                        self._adj_params_commit(par, cp)
                self._adj_step(w, u, P, rpp, "dopri5", 1, S, h_dev=cp, ctl=cp, c_out=c_sol, c_err=c_err, keep=keep, interp=ip)
                pn = self._adj_params_norm(par, 2, cp) if par else None
                self._adj_norm_control(w["ERR"], None, w, None, 2, P, rpp, ctl, pn)
                attempts += 1
            if ctx.get("adj_ctl_host"):
                self.ctl.posted(ctx, P)
            else:
                self.ctl.post(ctx, P, ctl)
            c = self.ctl.read(ctx, P, self.before_wait)
            if c is None:             # (inside a hipGraph capture nothing is posted)
                c = ctl.cpu()
            if all(bool(c[p, CTL_DONE] > 0) for p in range(P)):
                break
            if attempts >= self.ADJ_MAX_ATTEMPTS:
                raise _lib.NlbacError("odeint_adjoint (dopri5): max_num_steps exceeded")
            chain = 2
        used = int(max(float(c[p, CTL_NSTEPS]) for p in range(P)))       # attempts of the slowest problem
        self._adj_chain = max(1, used)
        ctx["adjoint_info"] = [[(float(c[p, CTL_HUSED]), float(c[p, CTL_RATIO]), int(c[p, CTL_NSTEPS]))
                                for p in range(P)]]
        # the interpolant of the last accepted step at t0 (steps are not clipped), all columns of z at once: written by
        # the attempt that finished each problem (interp), or by a launch of its own
        if not ip:
            _lib.call("nlbac_dopri_interp_fwd", w["Z0"].data_ptr(), w["Z1"].data_ptr(), KZ.data_ptr(), None, None, cp, P,
                      rpp, w["W"], w["OUT"].data_ptr(), 0, None, s)
        if par:
            self._adj_params_finish(par, cp)
        return w["OUT"]


class ConcatAdjoint(AffineAdjoint):
    """Continuous adjoint of the single-net field ``dx/dt = net([x, c])``."""
    # The base class drives the solve (initial step, attempts, mixed norm, commit, interpolation, parameter-adjoint
    # quadrature); what differs is one RK step of the augmented system z = [y | a_y | a_c] and the stage derivative of
    # the parameter adjoint: stage by stage on the MLP entry points (nlbac_concat_adj_in -> nlbac_mlp_fwd ->
    # nlbac_mlp_bwd_data -> nlbac_concat_adj_out), the RK combinations by nlbac_rk_combine on the w-wide rows.
    def _init_adjoint(self):
        super()._init_adjoint()
        self.adj_fused = None      # nlbac_concat_adj_step_ok of the net, asked at first use unless assigned (``_adj_fused``)

    def _adj_scratch(self, n, S):
        net, ns, nc = self.net, self.n_s, self.n_u
        return dict(ZS=self._buf("cadj_ZS", n, 2 * ns + nc), Xin=self._buf("cadj_Xin", n, net.in_dim),
                    Ay=self._buf("cadj_Ay", n, ns), f=self._buf("cadj_f", n, ns), dX=self._buf("cadj_dX", n, net.in_dim),
                    acts=self._buf("cadj_acts", net.n_layers - 1, n, net.hid))

    def _adj_fused(self):
        """One nlbac_concat_adj_step launch per attempted step (the reference's depth at widths 64 / 100 / 128);
        ``adj_fused = False`` keeps the stage-by-stage launches (other shapes; the cross-check)."""
        f = self.adj_fused
        if f is None:
            f = self.adj_fused = bool(_lib.load().nlbac_concat_adj_step_ok(C.byref(self.net.desc)))
        return f

    def _adj_interp_fold(self):
        return self._adj_fused() and self.interp_fold

    def _adj_step(self, w, u, P, rpp, method, st0, st1, h_host=None, h_dev=None, ctl=None, c_out=None, c_err=None,
                  keep=None, interp=False):
        """(Stage by stage: problems whose solve is done are recomputed to the same values — their control block, z0
        and first stage no longer change — instead of being skipped; the fused launch leaves their rows alone.)"""
        if self._adj_fused():
            beta, S = self._beta(method)
            k = keep or {}
            dp = lambda t: t.data_ptr() if t is not None else None
            _lib.call("nlbac_concat_adj_step", C.byref(self.net.desc), u.data_ptr(), P, rpp, st0, st1, S, beta,
                      c_out, len(c_out) if c_out is not None else 0, c_err, len(c_err) if c_err is not None else 0,
                      fptr(*h_host) if h_host is not None else None, h_dev, _lib.DOPRI_CTL if h_dev else 0, ctl,
                      w["Z0"].data_ptr(), w["KZ"].data_ptr(), w["Z1"].data_ptr() if c_out is not None else None,
                      w["ERR"].data_ptr() if c_err is not None else None,
                      self.norm.data_ptr() if self.norm is not None else None, dp(k.get("Xin")), dp(k.get("Ay")),
                      dp(k.get("acts")), k.get("ls", 0), dp(k.get("dz")), w["OUT"].data_ptr() if interp else None,
                      self.ctx["t_end"], stream_ptr())
            self.nfe += st1 - st0
            if keep:
                for st in range(st0, st1):
                    self._adj_stage_dw(self._adj_par_cur, st)
            return
        n, W, ns, nc, net, s = P * rpp, w["W"], self.n_s, self.n_u, self.net, stream_ptr()
        rows = TABLEAU[method]["beta"]
        S = len(rows) + 1
        sc = self._adj_scratch(n, S)
        hh = fptr(*h_host) if h_host is not None else None
        stride = _lib.DOPRI_CTL if h_dev else 0
        norm = self.norm.data_ptr() if self.norm is not None else None
        KZ = w["KZ"]
        for st in range(st0, st1):
            if st == 0:
                ZS = w["Z0"]
            else:
                ZS = sc["ZS"]
                _lib.call("nlbac_rk_combine", w["Z0"].data_ptr(), KZ.data_ptr(), st, fptr(*rows[st - 1]), hh, h_dev, stride,
                          P, rpp, W, ZS.data_ptr(), s)
            if keep:      # the parameter adjoint's quadrature reads every stage's net inputs / cotangents / activations
                Xin, Ay = keep["Xin"][st], keep["Ay"][st]
                acts, dz, ls = keep["acts"][:, st * n:], keep["dz"][:, st * n:], keep["ls"]
            else:
                Xin, Ay, acts, dz, ls = sc["Xin"], sc["Ay"], sc["acts"], None, n * net.hid
            _lib.call("nlbac_concat_adj_in", ZS.data_ptr(), W, u.data_ptr(), ns, nc, norm, n, Xin.data_ptr(), Ay.data_ptr(), s)
            io = io_array(1)
            io[0].x0, io[0].x0_dim, io[0].x0_ld = Xin.data_ptr(), net.in_dim, net.in_dim
            io[0].y, io[0].y_ld = sc["f"].data_ptr(), ns
            io[0].acts, io[0].acts_ls = acts.data_ptr(), ls
            _lib.call("nlbac_mlp_fwd", self._nets(), io, 1, n, s)
            io[0].dy, io[0].dy_ld = Ay.data_ptr(), ns
            io[0].dx, io[0].dx_ld = sc["dX"].data_ptr(), net.in_dim
            if dz is not None:
                io[0].dz = dz.data_ptr()
            _lib.call("nlbac_mlp_bwd_data", self._nets(), io, 1, n, s)
            _lib.call("nlbac_concat_adj_out", sc["f"].data_ptr(), sc["dX"].data_ptr(), ns, nc, norm, n, W, KZ[st].data_ptr(), s)
            if keep:
                self._adj_stage_dw(self._adj_par_cur, st)
        if c_out is not None:
            _lib.call("nlbac_rk_combine", w["Z0"].data_ptr(), KZ.data_ptr(), len(c_out), c_out, hh, h_dev, stride, P, rpp, W,
                      w["Z1"].data_ptr(), s)
        if c_err is not None:
            _lib.call("nlbac_rk_combine", None, KZ.data_ptr(), len(c_err), c_err, hh, h_dev, stride, P, rpp, W,
                      w["ERR"].data_ptr(), s)
        self.nfe += st1 - st0

    def _adj_keep(self, z, w, n, S):
        net, ns = self.net, self.n_s
        return dict(Xin=z(S, n, net.in_dim), Ay=z(S, n, ns), acts=z(net.n_layers - 1, S * n, net.hid),
                    dz=z(net.n_layers - 1, S * n, net.hid), ls=S * n * net.hid)

    def _adj_stage_dw(self, par, st):
        """K_theta[st] = sum over the rows of stage ``st`` of (d net / d theta)^T (a_y out_sig) at the stage's
        (normalised) inputs: nlbac_mlp_bwd_weights on what the step kept of that stage, then the slab sum."""
        k, n, S, net = par["keep"], par["n"], par["S"], self.net
        io = par["io"].get(st)
        if io is None:
            io = par["io"][st] = io_array(1)
            io[0].x0, io[0].x0_dim, io[0].x0_ld = k["Xin"][st].data_ptr(), net.in_dim, net.in_dim
            io[0].dy, io[0].dy_ld = k["Ay"][st].data_ptr(), self.n_s
            io[0].acts, io[0].dz = k["acts"][:, st * n:].data_ptr(), k["dz"][:, st * n:].data_ptr()
            io[0].acts_ls = S * n * net.hid
            io[0].grad = par["slabs"].data_ptr()
        bwd_weights(self._nets(), io, 1, n, self.ADJ_SUB_SLABS, par["NP"], self.device)
        _lib.call("nlbac_reduce_slabs", par["K"][st].data_ptr(), par["slabs"].data_ptr(), self.ADJ_SUB_SLABS,
                  par["NP"], par["NP"], stream_ptr())
        if self.comm is not None and self.comm.world > 1:
            self.comm.all_reduce_(par["K"][st])       # (see AffineNodeSolver._adj_stage_dw)
