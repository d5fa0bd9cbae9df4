"""dopri5's adaptive step control, the host half (``DopriDriver``, a base class of ``odeint.AffineNodeSolver``): the
norm and controller launches, the two ways an attempted step is driven — by the host, one accept decision per attempt
(ragged row counts; problems that diverge are finished by per-problem child solvers), or as a device-driven chain the
host looks at once — and every read of the control block (``ode_consts.CTL_*``).  It uses the solver's launch wrappers
(``_rk_fused``, ``_rk_fused_bwd``, ``_stage_eval``), its scratch buffers and step slots (``ode_workspace``), its
control-block reader (``ode_ctl``) and the solve's ``ctx``."""
import ctypes as C

import torch

from . import _lib
from ._lib import fptr
from .arena import stream_ptr
from .ode_consts import (CTL_ACCEPT, CTL_DONE, CTL_H0, CTL_HUSED, CTL_NACC, CTL_NSTEPS, CTL_OVF, CTL_RATIO, CTL_X, DP_BETA,
                         DP_C_ERR, ctl_field_ptr)


def ctl_column(c, P, field):
    """``field`` (a ``CTL_*``) of every problem, from ``c``: a host copy of the control block as nested lists
    (``.tolist()``: plain floats, see ``first_step_done``)."""
    return [c[p][field] for p in range(P)]


def ctl_info(c, P, accepted=None):
    """The record of one attempted step, per problem (step size tried, error ratio, accepted), from ``c`` as above;
    ``accepted``: the per-problem flags, None: every problem accepted."""
    return [(c[p][CTL_HUSED], c[p][CTL_RATIO], True if accepted is None else accepted[p]) for p in range(P)]


class DopriDriver:
    """The dopri5 half of a solver: attempts, accept decisions, the per-problem fallback and the chain's backward."""

    # -- control-block access ------------------------------------------------------------------------------------------
    def _ctl(self, P):
        return self._buf("ctl", P, _lib.DOPRI_CTL, dtype=torch.float64)

    def _ctl_post(self, P):
        self.ctl.post(self.ctx, P, self._ctl(P))

    def _ctl_read(self, P):
        """Host copy of the control block of the last attempted step (``ode_ctl``; inside a replayed hipGraph nothing
        was posted: the device block is read)."""
        c = self.ctl.read(self.ctx, P, self.before_wait)
        return c if c is not None else self._ctl(P).cpu()

    def first_step_done(self):
        """dopri5, after forward_begin: True iff every problem accepted its first step and reached dt
        (the overwhelmingly common case at dt=0.02).  One small D2H read."""
        P = self.ctx["P"]
        c = self._ctl_read(P)
        self.ctx["ctl_host"] = c
        cl = c.tolist()                 # (plain floats: element-wise reads of a tensor cost microseconds each, on the host's
        #                                  way from the accept decision to the launches that wait for it)
        if self.ctx.get("chain"):       # device-driven chain: every problem finished within the attempts enqueued
            ok = all(cl[p][CTL_DONE] > 0 and not cl[p][CTL_OVF] > 0 for p in range(P))
            if not ok:                  # a captured chain that is too short: later captures enqueue more attempts
                self._chain_len = int(max(ctl_column(cl, P, CTL_NSTEPS))) + 1
                self.generation += 1
            return ok
        return all(cl[p][CTL_ACCEPT] > 0 and cl[p][CTL_DONE] > 0 for p in range(P))

    def _dopri_finish(self, assume_single_step=False):
        """``forward_finish`` of a dopri5 solve."""
        if self.ctx.get("chain"):
            return self._dopri_finish_chain(assume_done=assume_single_step)
        if assume_single_step:
            return self._dopri_accept_first(None)
        return self._dopri_continue()

    # -- norm and step-size controller ---------------------------------------------------------------------------------
    def _norm_control(self, a, b, y0, y1, u, mode, P, rpp, slot_ctl=None, slot_floats=0, chain=None):
        """Scaled RMS norm(s) of mode 0/1/2 (include/nlbac_hip.h) over each problem's rows, then the step-size
        controller: one launch on a single GPU, norm -> all-reduce -> controller under data parallelism."""
        ctx = self.ctx
        ns, nu, s = self.n_s, self.n_u, stream_ptr()
        nblk = (rpp + 255) // 256
        part = self._buf("part", P, nblk, 2)
        ctl = self._ctl(P)
        dp = lambda t: t.data_ptr() if t is not None else None
        if self.comm is not None and self.comm.world > 1:
            _lib.call("nlbac_dopri_norm_partials", dp(a), dp(b), dp(y0), dp(y1), dp(u), mode, ctx["rtol"], ctx["atol"],
                      ns, nu, rpp, P, part.data_ptr(), slot_ctl, slot_floats, s)
            self._control(part, nblk, mode, P, rpp, ctx["t_end"], ctl, chain)
            return
        tickets = self._buf("tickets", P, dtype=torch.int32)
        _lib.call("nlbac_dopri_norm_control", dp(a), dp(b), dp(y0), dp(y1), dp(u), mode, ctx["rtol"], ctx["atol"],
                  ns, nu, rpp, P, ctx["t_end"], part.data_ptr(), tickets.data_ptr(), ctl.data_ptr(),
                  C.byref(chain) if chain is not None else None, s)

    def _control(self, part, nblk, mode, P, rpp, t_end, ctl, chain=None):
        """Step-size controller; under data parallelism the squared-norm sums are all-reduced first so every
        rank takes the decision the single-device run over the global batch would take."""
        ns, nu, s = self.n_s, self.n_u, stream_ptr()
        if self.comm is not None and self.comm.world > 1:
            sums = self._buf("psum", P, 1, 2)
            for p in range(P):
                _lib.call("nlbac_sum_partials", part[p].data_ptr(), nblk, 2, 1.0, sums[p].data_ptr(), s)
            self.comm.all_reduce_(sums)
            tail = (chain.n_slots, chain.hslots, chain.alog, chain.alog_cap) if chain is not None else (0, None, None, 0)
            _lib.call("nlbac_dopri_control", sums.data_ptr(), 1, mode, ns, nu, rpp * self.comm.world, P, t_end,
                      ctl.data_ptr(), *tail, s)
        else:
            _lib.call("nlbac_dopri_control", part.data_ptr(), nblk, mode, ns, nu, rpp, P, t_end, ctl.data_ptr(), 0, None,
                      None, 0, s)

    def _coef(self, key):
        c = self._coefs.get(key)
        if c is None:
            vals = DP_C_ERR if key == "err" else ([1.0] if key == "one" else (DP_BETA[5] + [0.0] if key == "sol" else
                                                                              DP_BETA[key[1] - 1]))
            c = self._coefs[key] = fptr(*vals)
        return c

    # -- host-driven attempts (ragged row counts) and the per-problem fallback -----------------------------------------
    def _dopri_begin(self, y0, u, P, rpp):
        if self._chain_ok(P, rpp):
            return self._dopri_begin_chain(y0, u, P, rpp)
        n, ns, nu, S = P * rpp, self.n_s, self.n_u, 7
        s = stream_ptr()
        ctl = self._ctl(P)
        ws = self._step_ws(n, S, 0)
        # f0 and the initial step size (Hairer's rule)
        if self.fused:
            self._rk_fused(ws, y0, u, P, rpp, "dopri5", 0, 1, h_dev=ctl.data_ptr())
        else:
            ws.Y[0].copy_(y0)
            self._stage_eval(ws, 0, u)
        self._norm_control(ws.K[0], None, y0, None, u, 0, P, rpp)
        h0_dev = ctl_field_ptr(ctl.data_ptr(), CTL_H0)
        if self.fused:
            # probe f(y0 + h0 f0): the fused kernel forms the stage input itself (same arithmetic as nlbac_rk_combine);
            # K[1] / Y[1] / gout[1] of the step workspace are scratch until the real stage 1 overwrites them
            self._rk_fused(ws, y0, u, P, rpp, "probe", 1, 2, h_dev=h0_dev, save_acts=False)
            ktmp = ws.K[1]
        else:
            ytmp, ktmp, gtmp = self._buf("ytmp", n, ns), self._buf("ktmp", n, ns), self._buf("gtmp", n, ns * nu)
            _lib.call("nlbac_rk_combine", y0.data_ptr(), ws.K.data_ptr(), 1, self._coef("one"), None, h0_dev,
                      _lib.DOPRI_CTL, P, rpp, ns, ytmp.data_ptr(), s)
            self._probe_eval(ytmp, u, n, ktmp, gtmp)
        self._norm_control(ktmp, ws.K[0], y0, None, None, 1, P, rpp)
        self._dopri_attempt(ws, y0, u, P, rpp)

    def _dopri_attempt(self, ws, cur_y0, u, P, rpp):
        """Stages 1..6 of one attempted step, error estimate, norm and controller (all on the device)."""
        ns, S = self.n_s, 7
        s = stream_ptr()
        h_dev = self._ctl(P).data_ptr()           # (CTL_H: the block's first field)
        if self.fused:
            self._rk_fused(ws, cur_y0, u, P, rpp, "dopri5", 1, S, h_dev=h_dev, c_err=self._coef("err"), err=ws.err)
        else:
            for st in range(1, S):
                _lib.call("nlbac_rk_combine", cur_y0.data_ptr(), ws.K.data_ptr(), st, self._coef(("b", st)), None,
                          h_dev, _lib.DOPRI_CTL, P, rpp, ns, ws.Y[st].data_ptr(), s)
                self._stage_eval(ws, st, u)
            _lib.call("nlbac_rk_combine", None, ws.K.data_ptr(), S, self._coef("err"), None, h_dev, _lib.DOPRI_CTL,
                      P, rpp, ns, ws.err.data_ptr(), s)
        self._norm_control(ws.err, None, cur_y0, ws.Y[6], None, 2, P, rpp)
        self._ctl_post(P)

    def _dopri_accept_first(self, c):
        """First step accepted and past dt: interpolate.  Step size and abscissa are read from the device
        control block by the kernels (identical arithmetic with or without a host copy of them).  ``c``: the host copy
        as nested lists, or None (no host copy: inside a hipGraph capture)."""
        ctx = self.ctx
        self.stats["single_step"] += 1
        P, rpp, n, ns = ctx["P"], ctx["rpp"], ctx["n"], self.n_s
        ws = self._step_ws(n, 7, 0)
        ctl = self._ctl(P)
        out = self._out_buf(n)       # (y1 is the input of stage 6: read in place, no copy)
        _lib.call("nlbac_dopri_interp_fwd", ctx["y0"].data_ptr(), ws.Y[6].data_ptr(), ws.K.data_ptr(), None, None,
                  ctl.data_ptr(), P, rpp, ns, out.data_ptr(), 0, None, stream_ptr())
        step = dict(ws=ws, first=True, dev=True)
        if c is not None:
            step["h"] = ctl_column(c, P, CTL_HUSED)
            step["x"] = ctl_column(c, P, CTL_X)
            ctx["info"] = [ctl_info(c, P)]
        ctx.update(steps=[step], out=out)
        return out

    def _dopri_continue(self, resume=None):
        """The attempt loop after the first attempted step has been queued.  ``resume``: state taken over from a joint
        solve (accepted steps so far, index of the step being attempted, attempt number) — see ``_adopt``."""
        ctx = self.ctx
        P, rpp, n, u, y0 = ctx["P"], ctx["rpp"], ctx["n"], ctx["u"], ctx["y0"]
        ns, S = self.n_s, 7
        s = stream_ptr()
        ctl = self._ctl(P)
        steps, info = [], []
        cur_y0, idx, start = y0, 0, 0
        if resume is not None:
            steps, info, cur_y0, idx, start = (resume["steps"], resume["info"], resume["cur_y0"], resume["idx"],
                                               resume["attempt"])
        ws = self._step_ws(n, S, idx)
        for attempt in range(start, 1000):
            c = ctx.pop("ctl_host", None)
            if c is None:
                c = self._ctl_read(P)             # the one host wait per attempted step
            cl = c.tolist()                       # (plain floats: see first_step_done)
            acc = [cl[p][CTL_ACCEPT] > 0 for p in range(P)]
            done = [cl[p][CTL_DONE] > 0 for p in range(P)]
            if any(a != acc[0] for a in acc) or any(d != done[0] for d in done):
                return self._solve_split(c, dict(steps=steps, info=info, idx=idx, attempt=attempt))
            if attempt == 0 and acc[0] and done[0]:
                return self._dopri_accept_first(cl)
            info.append(ctl_info(cl, P, acc))
            if attempt == 0:
                self.stats["multi_attempt"] += 1
            if acc[0]:
                steps.append(dict(ws=ws, h=ctl_column(cl, P, CTL_HUSED), first=(idx == 0)))
                if done[0]:
                    x = ctl_column(cl, P, CTL_X)
                    steps[-1]["x"] = x
                    out = self._out_buf(n)
                    _lib.call("nlbac_dopri_interp_fwd", cur_y0.data_ptr(), ws.Y[6].data_ptr(), ws.K.data_ptr(),
                              fptr(*steps[-1]["h"]), fptr(*x), None, P, rpp, ns, out.data_ptr(), 0, None, s)
                    ctx.update(steps=steps, out=out, info=info)
                    return out
                cur_y0 = ws.Y[6]                  # y1 of an accepted step = its stage-6 input (ws is not reused)
                idx += 1
                prev = ws
                ws = self._step_ws(n, S, idx)
                ws.Y[0].copy_(prev.Y[6])
                ws.K[0].copy_(prev.K[6])          # FSAL
            self._dopri_attempt(ws, cur_y0, u, P, rpp)
        raise _lib.NlbacError("dopri5: max_num_steps exceeded")

    def _adopt(self, k, p, c, st):
        """Hand per-problem solver ``k`` everything the joint solve has done for problem ``p``: its rows of every step
        workspace so far (stage derivatives, stage inputs, g(x), error estimate, activations / ReLU masks — one
        strided-copy launch per buffer) and its control block, so that it continues from the accept decision ``c``
        instead of starting the solve again.  Returns the state ``k._dopri_continue`` resumes from."""
        ctx = self.ctx
        P, rpp, n, S = ctx["P"], ctx["rpp"], ctx["n"], 7
        rows = slice(p * rpp, (p + 1) * rpp)
        k._touch(rpp)
        k.stats["solves"] += 1
        k.ctx = dict(method="dopri5", P=1, rpp=rpp, n=rpp, u=ctx["u"][rows], y0=ctx["y0"][rows], steps=[],
                     t_end=ctx["t_end"], atol=ctx["atol"], rtol=ctx["rtol"])
        s = stream_ptr()
        kws = []
        for j in range(st["idx"] + 1):                    # accepted steps 0 .. idx-1 and the step being attempted
            src, dst = self._step_ws(n, S, j), k._step_ws(rpp, S, j)
            for name in src.ADOPT:
                a, b = getattr(src, name), getattr(dst, name)
                w = a.shape[-1]                           # [.., rows, w] with rows = n or S*n (stage-major)
                _lib.call("nlbac_copy_blocks", a.data_ptr() + 4 * p * rpp * w, n * w, b.data_ptr(), rpp * w, rpp * w,
                          a.numel() // (n * w), s)
            kws.append(dst)
        _lib.call("nlbac_copy_blocks", self._ctl(P).data_ptr() + 8 * _lib.DOPRI_CTL * p, 2 * _lib.DOPRI_CTL,
                  k._ctl(1).data_ptr(), 2 * _lib.DOPRI_CTL, 2 * _lib.DOPRI_CTL, 1, s)
        k.ctx["ctl_host"] = c[p:p + 1].clone()
        steps = [dict(ws=kws[j], h=[step["h"][p]], first=step["first"]) for j, step in enumerate(st["steps"])]
        return dict(steps=steps, info=[[e[p]] for e in st["info"]], idx=st["idx"], attempt=st["attempt"],
                    cur_y0=kws[st["idx"] - 1].Y[6] if st["idx"] else k.ctx["y0"])

    def _solve_split(self, c, st):
        """The problems of one batch want different step sequences (one accepted / finished, another not): each has its
        own adaptive step size in the reference too (separate odeint calls), so the solve is finished problem by
        problem by child solvers on the row ranges, which take over what has been done jointly (``_adopt``; ``c``: host
        copy of the control block, ``st``: accepted steps / attempt number at the point of disagreement)."""
        ctx = self.ctx
        self.stats["split"] += 1
        P, rpp, n = ctx["P"], ctx["rpp"], ctx["n"]
        out = self._out_buf(n)
        kids, info = [], []
        for p in range(P):
            k = self._child(p)
            rows = slice(p * rpp, (p + 1) * rpp)
            if p == 0:
                key = "adopted" if st["attempt"] == 0 else "adopted_late"
                self.stats[key] = self.stats.get(key, 0) + 1
            o = k._dopri_continue(self._adopt(k, p, c, st))
            _lib.call("nlbac_copy_blocks", o.data_ptr(), o.numel(), out.data_ptr() + 4 * p * rpp * self.n_s, o.numel(),
                      o.numel(), 1, stream_ptr())
            kids.append(k)
            info.append(k.ctx.get("info"))
        ctx.update(split=kids, out=out, steps=[], info_split=info)
        ctx.pop("info", None)
        return out

    def _backward_split(self, dout, need_du, need_params, need_dy0):
        """``backward`` of a solve that was finished problem by problem (``_solve_split``)."""
        ctx = self.ctx
        assert not need_params, "parameter gradients are only taken on single-problem solves"
        rpp = ctx["rpp"]
        du = self._buf("du", ctx["n"], self.n_u) if need_du else None
        dy0 = self._buf("dy0_split", ctx["n"], self.n_s) if need_dy0 else None
        for p, k in enumerate(ctx["split"]):
            rows = slice(p * rpp, (p + 1) * rpp)
            du_p, dy0_p = k.backward(dout[rows], need_du=need_du, need_dy0=need_dy0)
            if du is not None:
                du[rows].copy_(du_p)
            if dy0 is not None:
                dy0[rows].copy_(dy0_p)
        return du, dy0

    def _child(self, p):
        """The per-problem solver of problem ``p`` (``reserve``, ``_solve_split``), with everything it takes from this
        solver — and nothing else: ``norm_defer``, ``interp_fold`` and ``row_groups`` stay at a child's own defaults
        (a child solves one problem on the host-driven path, which uses none of them)."""
        k = self._children.get(p)
        if k is None:
            k = self._children[p] = type(self)(self.node, self.device)
        k.comm, k.fused, k.keep_acts, k.fit_words = self.comm, self.fused, self.keep_acts, self.fit_words
        # the per-problem solvers run one after the other inside this solver's solve: they read through its read-back
        # stream and pinned blocks (a pinned allocation costs milliseconds)
        k.ctl = self.ctl
        k.before_wait = self.before_wait
        return k

    # -- dopri5 as a device-driven chain ------------------------------------------------------------------------
    # An attempted step is ONE launch: nlbac_node_rk_fwd with an nlbac_rk_chain description evaluates stages 1-6 in
    # the step slot the control block names, forms the error norm and runs the controller in its own epilogue.  The
    # host enqueues a fixed number of attempts (kernels skip problems that have finished) and looks at the control
    # block once per chain — not once per attempt; problems of one batch advance independently, so there is no
    # per-problem fallback on this path.  The backward walks the slots the same way (``back_idx``).
    ALOG_CAP = 64
    FUSED_NORM_MODES = (0, 1)

    def _chain_ok(self, P, rpp):
        return bool(self.device_loop and self.fused and (P == 1 or rpp % _lib.MLP_TILE == 0))

    def _chain(self, ws0, pool, P, rpp, norm_mode, read_ctl):
        ctx = self.ctx
        ctl = self._ctl(P)
        nblk = (rpp + _lib.MLP_TILE - 1) // _lib.MLP_TILE
        hs = self._buf("hslots%d" % pool.n_slots, P, pool.n_slots, dtype=torch.float64)
        c = _lib.RkChain()
        c.ctl = ctl.data_ptr() if read_ctl else None
        c.slot_floats, c.n_slots = pool.slot_floats, pool.n_slots
        c.rtol, c.atol, c.t_end = ctx["rtol"], ctx["atol"], ctx["t_end"]
        c.ctl_w, c.hslots = ctl.data_ptr(), hs.data_ptr()
        c.alog, c.alog_cap = self._buf("alog", P, self.ALOG_CAP, 3, dtype=torch.float64).data_ptr(), self.ALOG_CAP
        # the controller leaves the host's copy of the control block in pinned memory itself (see ControlBlockReader.posted)
        c.ctl_host = None if torch.cuda.is_current_stream_capturing() else self.ctl.io(P)[1].data_ptr()
        # Where the norm + controller run.  Fused into the RK launch's epilogue (last workgroup of a problem) for the two
        # one-stage launches of the initial-step selection: same GPU time as a launch of their own (26.7 us against
        # 18 + 9), one launch less each.  NOT for an attempted step: the epilogue's device-scope atomics queue behind the
        # six stages' stores (+18 us against a 9 us launch, MI355X) — it keeps the separate, slot-aware launch.  Data
        # parallel: always separate (the sums are all-reduced between the norm and the controller).
        if (self.comm is not None and self.comm.world > 1) or norm_mode not in self.FUSED_NORM_MODES:
            c.norm_mode = -1
        else:
            c.norm_mode = norm_mode
            c.partials = self._buf("cpart", P, nblk, 2).data_ptr()
            c.tickets = self._buf("ctickets", P, dtype=torch.int32).data_ptr()
        return c

    def _chain_control(self, ws0, pool, chain, y0, u, mode, P, rpp):
        """the scaled norm + step controller as launches of their own (slot-aware), where the RK launch did not run them
        in its epilogue (see ``_chain``)"""
        if chain.norm_mode >= 0 and not (mode == 2 and chain.norm_defer):
            return
        if chain.norm_mode >= 0:
            # an attempt whose RK launch left its tiles' partial sums (norm_defer): one small workgroup per problem
            if chain.ctl_host:
                chain.ctl_seq = self.ctl.next_stamp(self.ctx)
            _lib.call("nlbac_dopri_control_tiles", C.byref(chain), self.n_s, self.n_u, rpp, P, stream_ptr())
            return
        ctl = self._ctl(P)
        if mode == 0:
            self._norm_control(ws0.K[0], None, y0, None, u, 0, P, rpp)
        elif mode == 1:
            self._norm_control(ws0.K[1], ws0.K[0], y0, None, None, 1, P, rpp)
        else:
            if chain.ctl_host and not (self.comm is not None and self.comm.world > 1):
                chain.ctl_seq = self.ctl.next_stamp(self.ctx)
            self._norm_control(ws0.err, None, y0, ws0.Y[6], None, 2, P, rpp, slot_ctl=ctl.data_ptr(),
                               slot_floats=pool.slot_floats, chain=chain)

    def _dopri_begin_chain(self, y0, u, P, rpp, min_slots=1):
        n, S = P * rpp, 7
        ctx = self.ctx
        self.ctl.begin(ctx)           # (stamps of this solve's controller launches start here)
        pool = self._pool(n, S, min_slots)
        ws0 = pool.ws(n, 0)
        ctl = self._ctl(P)
        cp = ctl.data_ptr()
        ch = [self._chain(ws0, pool, P, rpp, m, read_ctl=(m == 2)) for m in (0, 1, 2)]
        ip, om = self._interp_fold(), self._out_map_fwd(n)
        if ip and om is not None and not self.OUT_MAP_IN_RK:
            ip = False                # (the single-net kernels evaluate no out-map)
        if ip:
            ch[2].interp_out = self._out_buf(n).data_ptr()
            if om is not None:
                ch[2].interp_kind, ch[2].interp_l, ch[2].interp_p = om.kind, om.l, om.p
        ctx["chain"] = dict(pool=pool, ws0=ws0, ch=ch[2], attempts=0, y0=y0, ip=ip, ip_om=om is not None)
        k = max(1, int(self._chain_len))
        if self._norm_defer_ok(ch):
            # The norms of f0 and of the probe without their elections (nlbac_rk_chain::norm_defer / norm_pre): each
            # launch leaves its tiles' partial sums, the NEXT launch's workgroups sum them and run the controller
            # themselves under their prologue's loads.
            nblk = (rpp + _lib.MLP_TILE - 1) // _lib.MLP_TILE
            part0, part1 = self._buf("cpart", P, nblk, 2).data_ptr(), self._buf("cpart1", P, nblk, 2).data_ptr()
            ch[0].norm_defer, ch[0].partials = 1, part0
            ch[1].norm_pre, ch[1].partials_pre, ch[1].norm_defer, ch[1].partials = 1, part0, 1, part1
            if self.norm_defer_attempt:
                # ... and the attempts': the RK launch leaves the error norm's tile partials, the controller launch is one
                # 64-thread workgroup per problem (nlbac_dopri_control_tiles) instead of a pass over the error rows
                ch[2].norm_mode, ch[2].norm_defer = 2, 1
                ch[2].partials = self._buf("cpart2", P, nblk, 2).data_ptr()
            first = _lib.RkChain.from_buffer_copy(ch[2])
            first.norm_pre, first.partials_pre = 2, part1
            ctx["chain"]["ch_first"] = first        # (the first attempted step only: later attempts get their step size from the controller launch)
        # f0 + Hairer's first guess, the probe f(y0 + h0 f0) + the initial step: one launch each (norms fused)
        self._rk_fused(ws0, y0, u, P, rpp, "dopri5", 0, 1, h_dev=cp, chain=ch[0])
        self._chain_control(ws0, pool, ch[0], y0, u, 0, P, rpp)
        self._rk_fused(ws0, y0, u, P, rpp, "probe", 1, 2, h_dev=ctl_field_ptr(cp, CTL_H0), save_acts=False,
                       chain=ch[1])
        self._chain_control(ws0, pool, ch[1], y0, u, 1, P, rpp)
        self._chain_attempts(k)

    def _norm_defer_ok(self, ch):
        """The election-free form of the two fused norms that open a dopri5 solve: where those norms are fused at all (one
        GPU) and the register-resident kernels serve the nets.  ``norm_defer = False`` (NLBAC_NORM_DEFER=0): the fused
        norms with their elections — the cross-check."""
        if not self.norm_defer or ch[0].norm_mode != 0 or ch[1].norm_mode != 1 or self._interp_nets()[1] is None:
            return False
        return bool(self._rr_kernels() and self.fused)

    def _chain_attempts(self, k):
        ctx = self.ctx
        st = ctx["chain"]
        P, rpp, u = ctx["P"], ctx["rpp"], ctx["u"]
        ws0, pool, ch = st["ws0"], st["pool"], st["ch"]
        cp = self._ctl(P).data_ptr()
        for _ in range(k):
            self._rk_fused(ws0, st["y0"], u, P, rpp, "dopri5", 1, 7, h_dev=cp, c_err=self._coef("err"), err=ws0.err,
                           chain=st.pop("ch_first", None) or ch)
            self._chain_control(ws0, pool, ch, st["y0"], u, 2, P, rpp)
        st["attempts"] += k
        if (self.comm is not None and self.comm.world > 1) or (ch.norm_mode == 2 and not ch.norm_defer):
            self._ctl_post(P)        # (the all-reduced controller is nlbac_dopri_control: it leaves no host copy; nor does
                                     #  the RK launch's own epilogue, FUSED_NORM_MODES with 2)
        else:
            self.ctl.posted(self.ctx, P)

    def _dopri_finish_chain(self, assume_done=False):
        ctx = self.ctx
        st = ctx["chain"]
        P, rpp, n, ns = ctx["P"], ctx["rpp"], ctx["n"], self.n_s
        pool, ws0 = st["pool"], st["ws0"]
        ctl = self._ctl(P)
        c = None
        while not assume_done:
            c = ctx.pop("ctl_host", None)
            if c is None:
                c = self._ctl_read(P)               # the one host wait per CHAIN of attempts
            c = c.tolist()                          # (plain floats: see first_step_done)
            if any(c[p][CTL_OVF] > 0 for p in range(P)):
                # out of step slots: the solve was stopped; start it again in a pool with room for twice as many steps
                self._dopri_begin_chain(ctx["y0"], ctx["u"], P, rpp, min_slots=2 * pool.n_slots)
                st = ctx["chain"]
                pool, ws0 = st["pool"], st["ws0"]
                continue
            if all(c[p][CTL_DONE] > 0 for p in range(P)):
                break
            if st["attempts"] >= 1000:
                raise _lib.NlbacError("dopri5: max_num_steps exceeded")
            self._chain_attempts(2)
        out = self._out_buf(n)
        if st.get("ip"):
            # the attempt that finished each problem has written its rows of `out` (and of the owner's map) itself
            ctx["out_mapped"] = st["ip_om"]
        else:
            # (the owner's map of the output — the Unicycle tasks' look-ahead point — is evaluated by this launch)
            om = self._out_map_fwd(n)
            _lib.call("nlbac_dopri_interp_fwd", ctx["y0"].data_ptr(), ws0.Y[6].data_ptr(), ws0.K.data_ptr(), None, None,
                      ctl.data_ptr(), P, rpp, ns, out.data_ptr(), pool.slot_floats, C.byref(om) if om is not None else None,
                      stream_ptr())
            ctx["out_mapped"] = om is not None
        if c is not None:
            nst = [int(v) for v in ctl_column(c, P, CTL_NSTEPS)]
            nacc = [int(v) for v in ctl_column(c, P, CTL_NACC)]
            self._chain_len = max(1, max(nst))
            key = "single_step" if max(nst) == 1 else "multi_attempt"
            self.stats[key] += 1
            alog = self._buf("alog", P, self.ALOG_CAP, 3, dtype=torch.float64).cpu() if max(nst) > 1 else None
            first = ctl_info(c, P)          # (a solve of single attempts: the control block still holds their record)
            info = []
            for k in range(min(max(nst), self.ALOG_CAP)):
                row = []
                for p in range(P):
                    if alog is None:
                        row.append(first[p])
                    elif k < nst[p]:
                        row.append((float(alog[p, k, 0]), float(alog[p, k, 1]), bool(alog[p, k, 2] > 0)))
                    else:
                        row.append(None)
                info.append(row)
            ctx.update(nacc=nacc, info=info)
            ctx["steps"] = [dict(ws=pool.ws(n, i), first=(i == 0)) for i in range(max(nacc) + 1)]
        else:
            ctx.update(nacc=None, steps=[dict(ws=ws0, first=True)])
        ctx["out"] = out
        return out

    def _backward_chain(self, dout, need_du, need_params, need_dy0):
        ctx = self.ctx
        st = ctx["chain"]
        P, rpp, n, u = ctx["P"], ctx["rpp"], ctx["n"], ctx["u"]
        ns, nu, s = self.n_s, self.n_u, stream_ptr()
        pool, ws0, ch = st["pool"], st["ws0"], st["ch"]
        ctl = self._ctl(P)
        # launches: one per accepted step of the slowest problem (unknown on the host inside a graph capture: then one
        # per attempt that was enqueued — launches beyond a problem's first step return at once)
        nb = (max(ctx["nacc"]) + 1) if ctx.get("nacc") is not None else st["attempts"]
        for i in range(nb):
            pool.ws(n, i).bwd(self)
        du = self._buf("du", n, nu) if need_du else None
        om = self._out_map_bwd(n) if dout is None else None
        assert dout is not None or om is not None, "backward(None) needs an output map (set_out_map) with its gradients"
        bch = _lib.RkChain()
        bch.ctl, bch.slot_floats, bch.n_slots, bch.hslots, bch.norm_mode = ch.ctl_w, pool.slot_floats, pool.n_slots, ch.hslots, -1
        if st.get("ip") and not (om is not None and not self.OUT_MAP_IN_RK):
            # the backward of the interpolant is the prologue of each problem's last-step launch (back_idx 0)
            bch.interp_bwd = 1
            if om is not None:
                bch.interp_kind, bch.interp_l, bch.interp_dp, bch.interp_dp2, bch.interp_x = om.kind, om.l, om.dp, om.dp2, om.x
            else:
                assert dout.is_contiguous() and dout.shape == (n, ns)
                bch.interp_dout = dout.data_ptr()
        else:
            _lib.call("nlbac_dopri_interp_bwd", dout.data_ptr() if dout is not None else None, None, None, ctl.data_ptr(), P,
                      rpp, ns, ws0.dy0.data_ptr(), ws0.dy1.data_ptr(), ws0.dK.data_ptr(), pool.slot_floats,
                      C.byref(om) if om is not None else None, s)
        for b in range(nb):
            self._rk_fused_bwd(ws0, u, P, rpp, "dopri5", True, need_dy0, need_params, None, None, 0, ws0.dy1, du,
                               b == 0, chain=bch, back_idx=b)
        return du, (ws0.dy0 if need_dy0 else None)

    def _rr_kernels(self):
        """The register-resident kernels serve the nets (nlbac_rk_interp_ok)."""
        ok = self._interp_ok
        if ok is None:
            ok = self._interp_ok = bool(_lib.load().nlbac_rk_interp_ok(*self._interp_nets()))
        return ok

    def _interp_fold(self):
        """The interpolation at t_end is evaluated by the attempt launches themselves and its backward by the last step's
        backward launch (nlbac_rk_chain::interp_*; the register-resident kernels): no nlbac_dopri_interp_fwd / _bwd
        launches.  ``interp_fold = False`` (NLBAC_INTERP_FOLD=0) keeps the two launches — the cross-check."""
        return bool(self.interp_fold and self._rr_kernels() and self.fused)
