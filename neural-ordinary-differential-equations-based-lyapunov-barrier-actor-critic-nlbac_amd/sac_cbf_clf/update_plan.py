"""What one update works on, built once per batch size: the minibatch row layout (``_Layout``), the device buffers
and per-update host state (``_Workspace``), the ctypes launch descriptors (``Plan``) with the pass that trades saved
activation rows for ReLU mask words (``keep_masks_drop_unpaired_acts``), and the captured hipGraphs (``GraphCache``).
``SAC_CBF_CLF`` (sac_cbf_clf.py) and the tasks (tasks.py) fill and launch these; nothing here launches a kernel.
"""
import ctypes as C

import torch

from .. import _lib
from ..arena import io_array, mlp_array, skinny_partials_ws
from . import _layout as SC


class _Layout:
    """Column offsets of one minibatch row in HBM: the fields of ``ReplayMemory.sample``
    (replay_memory.py:24-25) side by side, row stride padded to 16 bytes."""

    def __init__(self, task):
        self.obs_dim, self.act_dim, self.lya_dim = task.obs_dim, task.act_dim, task.lya_dim
        c = 0
        fields = [("obs", task.obs_dim), ("act", task.act_dim), ("rew", 1), ("con", 1), ("lya", task.lya_dim),
                  ("nlya", task.lya_dim), ("nobs", task.obs_dim), ("mask", 1), ("t", 1), ("nt", 1)]
        if task.has_signal:          # learned-barrier copies store a barrier signal after the constraint
            fields.insert(4, ("sig", 1))
        self.sig = None
        for name, w in fields:
            setattr(self, name, c)
            c += w
        self.width = c
        self.LD = (c + 3) // 4 * 4


class _Workspace:
    """Per-batch-size device buffers (allocated once, reused every update); the task adds its own."""

    def __init__(self, B, H, dev, lay, task):
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        A, Do = lay.act_dim, lay.obs_dim
        NP, NX = task.n_pol, task.n_extra_critics      # controllers; critic-type nets beyond Q1, Q2, L
        self.B = B
        self.mb = z(B, lay.LD)                   # minibatch rows (see _Layout)
        self.eps = z(task.n_eps, B, A)
        # policy samples of one update live side by side: rows [0,B) pi(s'), then pi(s) (and pi_backup(s)), so that
        # one forward launch and one sampling launch serve all of them
        self.heads3, self.act3, self.logp3 = z((1 + NP) * B, 2 * A), z((1 + NP) * B, A), z((1 + NP) * B)
        self.heads_n, self.na, self.nlogp = self.heads3[:B], self.act3[:B], self.logp3[:B]
        self.q6 = z(6 + 2 * NX, B)               # q1t q2t lt q1 q2 lf [xt x]...
        self.dq3 = z(3 + NX, B)
        self.next_q, self.next_l = z(B), z(B)
        self.acts_c = z(3 + NX, 2, B, H)         # Q1,Q2,L[,extras] saved activations
        self.dz_c = z(3 + NX, 2, B, H)
        self.nblk = (B + 255) // 256
        self.part_td = z(self.nblk, 3)
        self.n_tiles = (B + _lib.MLP_TILE_MIN - 1) // _lib.MLP_TILE_MIN
        self.part_td32 = z(self.n_tiles, 4)            # per-tile sums of the fused dy heads (nlbac_dy_head; 16-row tiles at most)
        # tickets of the heads' two-level elections: 1 + ceil(workgroups / 16) words each (TD head: <= 4 nets; actor head)
        self.tickets_td = torch.zeros(2 + self.n_tiles * 4 // 16 + 1, dtype=torch.int32, device=dev)
        self.tickets_q = torch.zeros(2 + self.n_tiles * NP // 16 + 1, dtype=torch.int32, device=dev)
        self.sums_tiles = torch.zeros(4, dtype=torch.int32, device=dev)    # nlbac_dy_head::sums_tiles of the td / actor-q heads
        self.sc_stage = z(SC.SC_SIZE)                                        # nlbac_dy_head::cb_stage
        self.part_tdx = z(max(NX, 1), self.nblk)
        self.heads2, self.pi2, self.logp2 = self.heads3[B:], self.act3[B:], self.logp3[B:]
        self.acts_p = z(NP, 2, B, H)
        self.dz_p = z(NP, 2, B, H)
        self.plan = {}                           # controllers updated -> Plan (SAC_CBF_CLF._plan)
        self.graphs, self.warm = GraphCache(task.solvers), 0
        self.qpi = z(2, NP * B)
        self.acts_q = z(2 * NP, 2, B, H)
        self.dq_pi = z(2, NP * B)
        self.part_q = z(NP, self.nblk, 2)
        self.part_q32 = z(NP, self.n_tiles, 2)
        self.dxq = z(2, NP * B, Do + A)
        self.dheads2 = z(NP * B, 2 * A)
        # --- host state of the update in flight (written by update_on_device and the pieces it runs) ---
        self._prefetched = None      # (update index, NP, targets piece queued?) of a draw + launches already queued
        self._pre_now = None         # ... the entry the current update consumed
        self._prefetch_fn = None     # the caller's draw (update_on_device(prefetch=...))
        self._sync = True            # the caller's ``sync``
        self.np_now, self.updates_now, self.blam_upd = task.n_pol, 0, 0     # controllers updated, update index, backup lambda step due
        self.q5_bwd_done = False     # the task ran the Q(s, pi) data backward inside one of its own launches
        self.p_part_q, self.n_part_q = None, 0      # where the actor step reads the Q(s, pi) sums (data parallel: all-reduced)
        self._mask_bufs = {}         # activation buffer address -> its ReLU mask words, shared by this workspace's plans
        task.alloc(self)


class GraphCache:
    """Captured hipGraphs by key.  All kernel arguments of a recorded launch sequence are static device pointers /
    constants (per-update scalars live in device memory).  A graph bakes in the addresses of the solvers' buffers and
    belongs to the solves it recorded: its entry keeps the solvers' ``generation`` (any freed or re-laid-out buffer
    invalidates it) and their solve contexts (restored before a replay, so that what the host does around the replay —
    reading the control block, finishing a solve eagerly — talks about THIS graph's solve and not about whichever
    batch size ran last)."""

    def __init__(self, solvers):
        self.solvers = solvers
        self.entries = {}          # key -> (graph, solver generations, [(solver, ctx, row count)])

    def __len__(self):
        return len(self.entries)

    def replay(self, key, fn):
        """Replay the graph of ``key``; ``fn``'s launches are recorded first if there is none yet or the solvers'
        buffers have moved since."""
        gens = tuple(sv.generation for sv in self.solvers)
        e = self.entries.get(key)
        if e is None or e[1] != gens:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            e = self.entries[key] = (g, tuple(sv.generation for sv in self.solvers),
                                     [(sv, sv.ctx, sv._cur_n) for sv in self.solvers])
        for sv, ctx, n in e[2]:
            if ctx is not None:
                sv.ctx, sv._cur_n = ctx, n
        e[0].replay()


def keep_masks_drop_unpaired_acts(io_arrays, bufs, alloc):
    """Where the register-resident MLP kernels serve the heads, every forward that saves something for a backward
    also leaves ReLU mask words (``nlbac_mlp_io::masks``, 64 B per row) and every data backward gates with them
    instead of loading the activation rows (24 float4 per lane at the head of each tile's critical path).  Nets that
    are only differentiated w.r.t. their inputs (Q(s, pi), V(p(x')), the barrier on predicted states: dx wanted, no
    dz / weight gradients) then keep nothing else — their activation buffer is dropped from the descriptors: the
    forward's 2 KB-per-row store burst goes.  Works on the finished launch descriptors of ALL of a plan's arrays: an
    activation buffer that no descriptor pairs with a dz, grad or skinny_ws buffer is such a net's.  ``bufs``:
    activation address -> mask buffer (anything with ``data_ptr()``), extended through ``alloc()``."""
    rows = {e.acts for arr in io_arrays for e in arr if e.acts and (e.dz or e.grad or e.skinny_ws)}
    for arr in io_arrays:
        for e in arr:
            if e.acts:
                if e.acts not in bufs:
                    bufs[e.acts] = alloc()
                e.masks = bufs[e.acts].data_ptr()
                if e.acts not in rows:
                    e.acts = None


def _addr(buf):
    return buf if buf is None or isinstance(buf, int) else buf.data_ptr()


def io_set(e, x0=None, x1=None, y=None, acts=None, dy=None, dx=None):
    """Fill one ``nlbac_mlp_io`` entry: ``x0`` / ``x1`` = (buffer, dim, ld) of an input block, ``y`` / ``dy`` / ``dx`` =
    (buffer, ld), ``acts`` = buffer.  A buffer is a tensor or a device address; what is not named stays as it is."""
    if x0 is not None:
        e.x0, e.x0_dim, e.x0_ld = _addr(x0[0]), x0[1], x0[2]
    if x1 is not None:
        e.x1, e.x1_dim, e.x1_ld = _addr(x1[0]), x1[1], x1[2]
    if y is not None:
        e.y, e.y_ld = _addr(y[0]), y[1]
    if acts is not None:
        e.acts = _addr(acts)
    if dy is not None:
        e.dy, e.dy_ld = _addr(dy[0]), dy[1]
    if dx is not None:
        e.dx, e.dx_ld = _addr(dx[0]), dx[1]


def io_copy_and_one(dst, src, n, last):
    """dst = src[:n] + last[:1]: the entries of one launch with one more net's entry behind them."""
    sz = C.sizeof(_lib.MlpIO)
    C.memmove(dst, src, n * sz)
    C.memmove(C.byref(dst, n * sz), last, sz)


def gauss_head(pol, eps, n_u, action, action_ld, logp):
    """The ``nlbac_gauss_head`` of a launch of policy nets that draws its own samples (launch folds on)."""
    gh = _lib.GaussHead()
    gh.eps, gh.scale, gh.bias, gh.n_u = eps.data_ptr(), pol.action_scale.data_ptr(), pol.action_bias.data_ptr(), n_u
    gh.action, gh.action_ld, gh.logp = action.data_ptr(), action_ld, logp.data_ptr()
    return gh


def actor_scalars_set(S, agent, NP):
    """Fill an ``nlbac_actor_scalar_args``: where log alpha and its gradient live, per controller updated."""
    S.target_entropy, S.sc = agent.target_entropy, agent.sc.data_ptr()
    for g in agent.actor_groups:
        for k in range(min(g.count, NP - g.first)):
            off = g.la_off + k * g.la_stride
            S.log_alpha[g.first + k] = g.arena.theta.data_ptr() + 4 * off
            S.g_log_alpha[g.first + k] = g.arena.grad.data_ptr() + 4 * off


class Plan:
    """ctypes launch arguments of one workspace: every pointer is static (arenas, workspace tensors) and every constant
    follows from the agent and its switches ``fold_launches`` / ``sums_defer`` as they stand when the plan is constructed,
    so all are built here, once (per number of controllers updated: Pvtol trains its backup every 20th update); an update
    is then a plain sequence of C calls.  Every ``nlbac_mlp_io`` array is made by ``io()``, which is how the mask pass
    finds them all — wherever the plan keeps them.  A head structure (the folded per-row steps) that the update will not
    use is None; a launch site stores only what changes per update.  The task's ``plan()`` adds its own arrays and heads."""

    def __init__(self, agent, ws, NP):
        self.io_arrays = []
        # per update: the augmented-Lagrangian step a task's constraint head left for the update's last MLP launch
        self.cf_job = None
        B, lay, task = ws.B, agent.lay, agent.task
        mb = ws.mb.data_ptr()
        LD, Do, Da, Dl = lay.LD, lay.obs_dim, lay.act_dim, lay.lya_dim
        col = lambda c: mb + 4 * c
        lc, lnc = task.lya_train_cols(lay)       # inputs the Lyapunov critic is regressed on
        p_obs, p_act, p_cen, p_ncen, p_nobs = col(lay.obs), col(lay.act), col(lc), col(lnc), col(lay.nobs)
        obs, nobs = (p_obs, Do, LD), (p_nobs, Do, LD)                      # input blocks (buffer, dim, ld) ...
        act, nact = (p_act, Da, LD), (ws.na, Da, Da)                       # ... stored / re-sampled next action
        P = self
        P.p_obs, P.p_rew, P.p_con, P.p_mask, P.LD = p_obs, col(lay.rew), col(lay.con), col(lay.mask), LD
        q1, q2, l, pi = agent.h_q1, agent.h_q2, agent.h_l, agent.h_p
        P.NP, NX = NP, len(agent.h_extra)
        # A: pi(s')
        P.n_pol, P.io_pol_next = mlp_array([pi.desc]), P.io(1)
        io_set(P.io_pol_next[0], x0=nobs, y=(ws.heads_n, 2 * Da))
        # A: targets + critic / Lyapunov forward (6 nets)
        descs = [q1.desc_target, q2.desc_target, l.desc_target, q1.desc, q2.desc, l.desc]
        for h in agent.h_extra:
            descs += [h.desc_target, h.desc]
        P.n_six, P.n_six_count = mlp_array(descs), len(descs)
        io = P.io_six = P.io(len(descs))
        for i in range(len(descs)):
            io_set(io[i], y=(ws.q6[i], 1))
        for k in range(NX):            # extra critic-type nets on (s', a') [target] and (s, a)
            io_set(io[6 + 2 * k], x0=nobs, x1=nact)
            io_set(io[7 + 2 * k], x0=obs, x1=act, acts=ws.acts_c[3 + k])
        for i in (0, 1):
            io_set(io[i], x0=nobs, x1=nact)
        io_set(io[2], x0=(p_ncen, Dl, LD))
        for i in (3, 4):
            io_set(io[i], x0=obs, x1=act, acts=ws.acts_c[i - 3])
        io_set(io[5], x0=(p_cen, Dl, LD), acts=ws.acts_c[2])
        # B: critic / Lyapunov backward
        P.n_crit = mlp_array([h.desc for h in agent.h_crit])
        io = P.io_crit = P.io(3 + NX)
        for i in range(3 + NX):
            io_set(io[i], acts=ws.acts_c[i], dy=(ws.dq3[i], 1))
            io[i].dz, io[i].grad = ws.dz_c[i].data_ptr(), agent.ar_c.grad.data_ptr()
        for i in [0, 1] + list(range(3, 3 + NX)):
            io_set(io[i], x0=obs, x1=act)
        io_set(io[2], x0=(p_cen, Dl, LD))
        # (its data backward leaves the skinny-gradient partial sums for the weight backward: one launch less)
        P.sk_crit = skinny_partials_ws(P.n_crit, (io,), 3 + NX, B, agent.device)
        # C: both actors (forward and backward share one descriptor)
        def act_io(io, j, i):            # entry j of an io array describes controller i
            io_set(io[j], x0=obs, y=(ws.heads2[i * B:], 2 * Da), acts=ws.acts_p[i], dy=(ws.dheads2[i * B:], 2 * Da))
            io[j].dz, io[j].grad = ws.dz_p[i].data_ptr(), agent.pol_arena[i].grad.data_ptr()
        P.n_act = mlp_array([h.desc for h in agent.h_pols[:NP]])
        io = P.io_act = P.io(NP)
        for i in range(NP):
            act_io(io, i, i)
        P.n_pol3 = mlp_array([pi.desc] + [h.desc for h in agent.h_pols[:NP]])     # pi(s') + the actors on s
        io3 = P.io_pol3 = P.io(1 + NP)
        io_set(io3[0], x0=nobs, y=(ws.heads_n, 2 * Da))
        for i in range(NP):
            act_io(io3, 1 + i, i)
        P.act_groups = []                # per Adam group: the nets whose weight gradients land in its arena
        for g in agent.actor_groups:
            cnt = min(g.count, NP - g.first)
            if cnt <= 0:
                continue
            gio = P.io(cnt)
            for j in range(cnt):
                act_io(gio, j, g.first + j)
            nets_g = mlp_array([h.desc for h in agent.h_pols[g.first:g.first + cnt]])
            # the actors' data backward (P.io_act) leaves this group's skinny-gradient partials for its weight backward
            io_act_g = [P.io_act[g.first + j] for j in range(cnt)]       # (views into the array, not copies)
            sk = skinny_partials_ws(nets_g, (gio, io_act_g), cnt, B, agent.device)
            P.act_groups.append((g, cnt, nets_g, gio, sk))
        # C: Q(s, pi) for primary / backup + V(current Lyapunov input)
        extra = task.extra_value_nets()
        P.n_q5 = mlp_array([q1.desc, q2.desc] * NP + [l.desc] + [h.desc for h in extra])
        P.n_q5_count = 2 * NP + 1 + len(extra)
        io = P.io_q5 = P.io(P.n_q5_count)
        for i in range(2 * NP):
            half = i // 2                                      # 0 primary, 1 backup
            io_set(io[i], x0=obs, x1=(ws.pi2[half * B:], Da, Da), y=(ws.qpi[i % 2, half * B:], 1), acts=ws.acts_q[i],
                   dy=(ws.dq_pi[i % 2, half * B:], 1), dx=(ws.dxq[i % 2, half * B:], Do + Da))
            io[i].dx_first = Do                                # (only dQ / da is consumed)
        task.value_now_io(ws, io, 2 * NP)
        task.extra_value_io(ws, io, 2 * NP + 1)
        P.heads(agent, ws)
        task.plan(ws, P)
        # mask words wherever the register-resident kernels serve the heads' launches (see the pass above).  The mask
        # buffer is sized for what those kernels take: two hidden layers of at most 256 units (8 words per row and layer)
        # (every net a descriptor of a plan names is one of these: Q1, Q2, L and the barrier net are ``h_crit`` — a task's
        #  ``a.h_l`` / ``a.h_extra[0]`` are its members —, the controllers ``h_pols``)
        nets = agent.h_crit + agent.h_pols
        if agent.fold_launches and _lib.load().nlbac_mlp_masks_ok(mlp_array([h.desc for h in nets]), len(nets)):
            assert all(h.n_layers == 3 and h.hid <= 256 for h in nets), "mask words: (2, B, 8) per net"
            keep_masks_drop_unpaired_acts(P.io_arrays, ws._mask_bufs,
                                          lambda: torch.zeros(2, B, 8, dtype=torch.int32, device=agent.device))

    def heads(self, agent, ws):
        """The head structures of the shared launches, each under the condition its launch site asks (sac_cbf_clf.py),
        and the constant part of ``nlbac_auglag``'s arguments."""
        P, task, lay, NP, B = self, agent.task, agent.lay, self.NP, ws.B
        A, Do, LD = lay.act_dim, lay.obs_dim, lay.LD
        G = B * agent.world                      # rows the batch means run over
        sc, q, tiles = agent.sc.data_ptr(), ws.q6, ws.sums_tiles.data_ptr()
        one, fold = agent.world == 1, agent.fold_launches
        # the batch sums of the td / actor-q dy heads (and of a task's constraint head) are finished by a workgroup of the
        # actors' data backward instead of by an election at the end of their own launches (nlbac_dy_head::sums_defer /
        # finish): single GPU with the launch folds.  ``agent.sums_defer = False`` (NLBAC_SUMS_DEFER=0): the elections
        P.sums_defer = bool(agent.sums_defer and one and fold)
        P.auglag = P.head_pol3 = P.head_td = P.actor_scalars = P.head_actor_q = P.head_gauss = None
        if one:                 # (SAC_CBF_CLF.auglag_fused stores the two lambda-update flags per update)
            L = P.auglag = _lib.AuglagArgs()
            L.n_cbf, L.n_clf, L.batch_size = task.num_cbfs, 1, float(agent.batch_size)
            L.ratio_mode, L.backup_mode = task.ratio_mode, task.backup_mode if NP == 2 else 0
            L.lam_lo, L.lam_hi = task.lam_lo, task.lam_hi
        if one and not fold:    # nlbac_actor_q_terms: its last workgroup runs nlbac_actor_scalars
            P.actor_scalars = _lib.ActorScalarArgs()
            actor_scalars_set(P.actor_scalars, agent, NP)
        if not fold:
            return
        # pi(s') + the actors on s: all (1 + NP) * B samples are drawn by the policy launch itself
        P.head_pol3 = gauss_head(agent.policy, ws.eps, A, ws.act3, A, ws.logp3)
        if one and len(agent.h_extra) <= 1:
            # dy head kind 2: targets, dL/dq and the three losses are produced by the critics' data backward itself
            H = P.head_td = _lib.DyHead()
            H.kind, H.B_norm = 2, G
            H.q1t, H.q2t, H.lt, H.nlogp = q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), ws.nlogp.data_ptr()
            H.reward, H.constraint, H.mask, H.rcm_ld = P.p_rew, P.p_con, P.p_mask, LD
            H.alpha, H.gamma = sc + 4 * SC.SC_ALPHA, agent.gamma
            for k in range(3):
                H.q[k], H.dq[k] = q[3 + k].data_ptr(), ws.dq3[k].data_ptr()
            H.next_q, H.next_l = ws.next_q.data_ptr(), ws.next_l.data_ptr()
            H.partials, H.ticket = ws.part_td32.data_ptr(), ws.tickets_td.data_ptr()
            H.mul, H.out = 1.0 / G, sc + 4 * SC.SC_QF1
            if P.sums_defer:    # no election: the launch's tiles leave their squared-error sums (finish[0] below)
                H.sums_defer, H.sums_tiles = 1, tiles
            if agent.h_extra:   # BarrierNet TD step (NU/sac_cbf_clf.py:224-233): the launch's 4th net
                H.xt, H.xq, H.dxq = q[6].data_ptr(), q[7].data_ptr(), ws.dq3[3].data_ptr()
                H.xsig, H.xsig_ld = ws.mb.data_ptr() + 4 * lay.sig, LD
                H.out_x = sc + 4 * SC.SC_XLOSS
        if one:
            # dy head kind 3 of the Q(s, pi) data backward: d min(Q1, Q2), policy_loss_1, the alpha losses, d log_alpha
            H = P.head_actor_q = _lib.DyHead()
            H.kind, H.B_norm, H.n_prob = 3, G, NP
            H.qa, H.qb, H.logp = ws.qpi[0].data_ptr(), ws.qpi[1].data_ptr(), ws.logp2.data_ptr()
            H.dqa, H.dqb = ws.dq_pi[0].data_ptr(), ws.dq_pi[1].data_ptr()
            H.alpha = sc + 4 * SC.SC_ALPHA
            actor_scalars_set(H.actor, agent, NP)
            H.partials, H.ticket = ws.part_q32.data_ptr(), ws.tickets_q.data_ptr()
            if P.sums_defer:
                H.sums_defer, H.sums_tiles = 1, tiles + 4
        # dy head kind 1 of the actors' data backward: d heads from d action (two Q nets; per update the rollout's) and d logp
        H = P.head_gauss = _lib.DyHead()
        H.kind, H.B_norm, H.scale, H.n_u = 1, G, agent.policy.action_scale.data_ptr(), A
        H.heads, H.heads_ld, H.eps = ws.heads2.data_ptr(), 2 * A, ws.eps[1:1 + NP].data_ptr()
        for k in (0, 1):
            H.da[k], H.da_ld[k] = ws.dxq[k].data_ptr() + 4 * Do, Do + A
        H.alpha, H.dlogp_mul = sc + 4 * SC.SC_ALPHA, 1.0 / G
        H.dheads, H.dheads_ld = ws.dheads2.data_ptr(), 2 * A
        # the sums the td head and the actor-q head left as tile partials (sums_defer): two workgroups of this launch
        # finish them — before the Adam step that reads d log_alpha and mirrors the losses
        deferred = [h for h in (P.head_td, P.head_actor_q) if h is not None and h.sums_defer]
        for F, src in zip(H.finish, deferred):
            F.kind, F.partials, F.n_tiles = src.kind, src.partials, src.sums_tiles
            if src.kind == 2:
                F.n_nets, F.mul, F.out, F.out_x = len(agent.h_crit), src.mul, src.out, src.out_x
            else:
                F.n_nets, F.B_norm = src.n_prob, src.B_norm
                C.memmove(C.byref(F.actor), C.byref(src.actor), C.sizeof(_lib.ActorScalarArgs))

    def io(self, n):
        """A zeroed ``nlbac_mlp_io[n]`` that belongs to this plan."""
        arr = io_array(n)
        self.io_arrays.append(arr)
        return arr
