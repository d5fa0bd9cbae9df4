"""``SAC_CBF_CLF`` — drop-in for the reference agent class (``U/sac_cbf_clf/sac_cbf_clf.py:26-656`` and its
per-environment copies ``C/``, ``P/``; the learned-barrier copies ``NU/``, ``NP/`` are the subclass in
``nlbac_amd/neural_barrier_certificate/``) whose ``update_parameters`` runs entirely on one MI355X through the C ABI
in ``include/nlbac_hip.h``.

Same constructor arguments, public methods, return values, checkpoint files and ``state_dict`` key names as the
reference.  Differences that are visible to a caller:
  * CUDA(HIP)-only: ``args.cuda`` must be true (no CPU fallback);
  * ``self.solver`` may be ``'euler'`` (reference default), ``'rk4'`` or ``'dopri5'``; the NODE-fit and CBF/CLF
    rollouts use it;
  * Lagrange multipliers / augmented terms / temperatures live on the device (``lambda_values`` etc. are read-back
    properties);
  * policy noise comes from the device generator unless ``set_noise`` is given pre-drawn N(0,1) samples (parity tests);
  * a replay object with ``sample_rows`` (``DeviceReplayMemory``) is gathered on the device.

The environment-specific half of an update (row layout, NODE form, rollout, CBF / CLF terms, NODE fit) is a task
object (``tasks.py``) chosen from ``env.dynamics_mode``; this file holds the shared SAC / Lyapunov machinery:
``_upd_part1`` (targets, critic step, actor forward, rollout start) and ``_upd_part2`` (constraints, actor backward,
actor step), see DESIGN.md §3.  What they work on — the per-batch-size workspace, the launch descriptors, the captured
hipGraphs — is ``update_plan.py``; how the returned floats reach the host, ``scalars_readback.py``.  Host<->device
traffic per update: the minibatch upload (or 8 bytes per row of indices), one 512-byte scalars read-back and, for
dopri5, one 256-byte control block per attempted step.
"""
import collections
import ctypes as C
import os
import random
import types

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..arena import Arena, bwd_weights, pack, stream_ptr
from ..node_fit import loss_blocks, node_fit_options, traj_mse_launch, valid_counts
from . import _layout as SC
from .model import BarrierNetwork, GaussianPolicy, LyaNetwork, QNetwork
from .scalars_readback import ScalarsReadback
from .tasks import TASKS
from .update_plan import GraphCache, Plan, _Layout, _Workspace
from .utils import to_tensor

DYNAMICS_MODE = {'Unicycle': {'n_s': 3, 'n_u': 2}, 'SimulatedCars': {'n_s': 10, 'n_u': 1},
                 'Pvtol': {'n_s': 6, 'n_u': 2}, 'Quadrotor': {'n_s': 6, 'n_u': 2}}
l_p = 0.03


class PoseLoss(nn.Module):
    """MSE('mean') — kept for API parity; the fit computes it on device."""

    def forward(self, predicted_state, true_state):
        return nn.functional.mse_loss(predicted_state, true_state)


class SAC_CBF_CLF(object):
    variant = ""         # "Barrier" in the learned-barrier-certificate copies (neural_barrier_certificate/)

    def __init__(self, num_inputs, action_space, env, args):
        self.gamma = args.gamma
        self.gamma_b = args.gamma_b
        self.tau = args.tau
        self.policy_type = args.policy
        self.batch_size = args.batch_size
        self.target_update_interval = args.target_update_interval
        self.Lagrangian_multiplier_update_interval = args.Lagrangian_multiplier_update_interval
        self.automatic_entropy_tuning = args.automatic_entropy_tuning
        self.action_space = action_space
        self.action_space.seed(args.seed)
        if not args.cuda or not torch.cuda.is_available():
            raise RuntimeError("nlbac_amd.SAC_CBF_CLF runs on an MI355X only (pass --cuda on a GPU box); "
                               "there is no CPU fallback")
        if self.policy_type != "Gaussian":
            raise NotImplementedError("only the Gaussian policy is on the device path")
        if env.dynamics_mode + self.variant not in TASKS:
            raise Exception('Dynamics mode not supported.')
        _lib.load()
        self.device = torch.device("cuda")
        self.env = env
        self.task = task = TASKS[env.dynamics_mode + self.variant](self, env, args)
        self.lay = _Layout(task)
        if num_inputs != task.obs_dim or action_space.shape[0] != task.act_dim:
            raise ValueError("%s expects %d observations / %d actions" % (task.name, task.obs_dim, task.act_dim))
        self.center_pos_num = task.lya_dim       # inputs of the Lyapunov network
        self.critic_lyapunov_lr = 0.0004
        self.lr = args.lr
        hidden = args.hidden_size
        n_act = action_space.shape[0]
        self.num_inputs, self.n_act, self.hidden = num_inputs, n_act, hidden
        # NODE fit over trajectory windows of ``node_horizon`` consecutive transitions (fit_node_windows); 1: the
        # reference's one-step fit, the path as it was.  ``node_stride``: replay rows between consecutive steps of one
        # trajectory (the lane count of a driver that pushes one row per lane per step)
        self.node_horizon, self.node_stride = node_fit_options(args)
        # gradient slabs of the actor / critic arenas (row ranges whose weight-gradient partials the optimiser sums).  8 for
        # the usual batches; 16 from batch 16384 on: a slab is then still >= 1024 rows and mlp_bwd_wide has twice the
        # workgroups (measured at B = 32768: 184 -> 159 us per launch; 128 x 128 output tiles instead — half the operand
        # re-reads — were slower than that, 170 us, and were dropped)
        self.n_grad_slabs = int(getattr(args, "grad_slabs", 16 if int(getattr(args, "batch_size", 0) or 0) >= 16384 else 8))
        if os.environ.get("NLBAC_GRAD_SLABS"):           # (experiments)
            self.n_grad_slabs = int(os.environ["NLBAC_GRAD_SLABS"])

        # --- same construction order (and RNG consumption) as the reference ---
        self.critic = QNetwork(num_inputs, n_act, hidden)
        self.lyapunovNet = LyaNetwork(self.center_pos_num, hidden)
        self.BarrierNet = BarrierNetwork(num_inputs, n_act, hidden) if task.has_signal else None
        QNetwork(num_inputs, n_act, hidden)          # the reference builds target nets here
        LyaNetwork(self.center_pos_num, hidden)      # (then hard-copies): consume the same RNG
        if task.has_signal:
            BarrierNetwork(num_inputs, n_act, hidden)
        self.cost_limit = 0.0
        self.augmented_ratio = 1.0005
        if args.seed >= 0:
            env.seed(args.seed)
            random.seed(args.seed)
            env.action_space.seed(args.seed)
            torch.manual_seed(args.seed)
            np.random.seed(args.seed)
            torch.cuda.manual_seed_all(args.seed)
        self.target_entropy = -float(np.prod(action_space.shape))
        self.log_alpha = nn.Parameter(torch.zeros(1))
        self.backup_log_alpha = nn.Parameter(torch.zeros(1))
        self.policy = GaussianPolicy(num_inputs, n_act, hidden, action_space)
        self.backup_policy = GaussianPolicy(num_inputs, n_act, hidden, action_space) if task.n_pol == 2 else None

        self.num_cbfs = task.num_cbfs
        self.l_p = l_p
        self.action_dim = env.action_space.shape[0]
        self.u_min, self.u_max = self.get_control_bounds()
        self.num_constraints = self.num_cbfs + 1
        self.neural_ode_model = task.build_node()
        self.solver = 'euler'
        self.model_loss_func = PoseLoss()
        self.atol, self.rtol = 1e-7, 1e-5

        # --- flat HBM arenas, one per optimiser group --------------------------
        dev = self.device
        self.ar_c = Arena(dev, self.n_grad_slabs, with_target=True)     # critic + Lyapunov (lr 4e-4)
        self.ar_a = Arena(dev, self.n_grad_slabs)                        # policies + log alphas (lr args.lr)
        self.n_fit_slabs = int(getattr(args, "fit_grad_slabs", 51))      # per accepted RK step of a NODE fit (row slabs = workgroups;
        # f_net + g_net have five hid x hid layers: 5 x 51 = 255 long workgroups for 256 CUs, mlp_dw16_kernels.hip)
        self.ar_n = Arena(dev, self.n_fit_slabs * 2)                     # NODE (lr 1e-3)
        self.h_q1, self.h_q2 = self.critic.attach(self.ar_c)
        (self.h_l,) = self.lyapunovNet.attach(self.ar_c)
        self.h_extra = list(self.BarrierNet.attach(self.ar_c)) if task.has_signal else []
        (self.h_p,) = self.policy.attach(self.ar_a)
        self.h_pols = [self.h_p]
        # a backup controller stepped on its own schedule (Pvtol: every 20th update) needs its own Adam state
        self.ar_b = Arena(dev, self.n_grad_slabs) if (task.n_pol == 2 and task.backup_interval > 1) else None
        ar_backup = self.ar_b if self.ar_b is not None else self.ar_a
        if task.n_pol == 2:
            (self.h_b,) = self.backup_policy.attach(ar_backup)
            self.h_pols.append(self.h_b)
        self.ar_a.add_group([self.log_alpha])
        if task.n_pol == 2:
            ar_backup.add_group([self.backup_log_alpha])
        self.h_node = list(self.neural_ode_model.attach(self.ar_n))
        self.arenas = [a for a in (self.ar_c, self.ar_a, self.ar_b, self.ar_n) if a is not None]
        for ar in self.arenas:
            ar.finalize()
        self.ar_c.hard_update_target()
        self.policy.to(dev)
        if self.backup_policy is not None:
            self.backup_policy.to(dev)
        self.h_crit = [self.h_q1, self.h_q2, self.h_l] + self.h_extra       # one Adam group, lr 4e-4
        for h in self.h_crit + self.h_pols + self.h_node:
            h.bind()
        la_off = self.ar_a.offset_of[id(self.log_alpha)]
        G = types.SimpleNamespace
        if self.ar_b is not None:       # two Adam groups: [policy, log_alpha] and [backup policy, backup log_alpha]
            self.actor_groups = [G(arena=self.ar_a, first=0, count=1, la_off=la_off, la_stride=0),
                                 G(arena=self.ar_b, first=1, count=1, la_stride=0,
                                   la_off=self.ar_b.offset_of[id(self.backup_log_alpha)])]
        else:
            stride = (self.ar_a.offset_of[id(self.backup_log_alpha)] - la_off) if task.n_pol == 2 else 0
            self.actor_groups = [G(arena=self.ar_a, first=0, count=task.n_pol, la_off=la_off, la_stride=stride)]
        self.pol_arena = [self.ar_a] + ([ar_backup] if task.n_pol == 2 else [])
        # target networks as modules over the Polyak buffer (state_dict / inspection)
        self.critic_target = _TargetView(self.critic, self.ar_c)
        self.lyapunovNet_target = _TargetView(self.lyapunovNet, self.ar_c)
        if task.has_signal:
            self.BarrierNet_target = _TargetView(self.BarrierNet, self.ar_c)
        self.repack_all()
        for ar in self.arenas:          # (built here, not inside a captured update)
            ar.scatter_tables()

        # --- device scalars: alpha, lambdas, augmented term --------------------
        self.sc = torch.zeros(SC.SC_SIZE, dtype=torch.float32, device=dev)
        sc_host = np.zeros(SC.SC_SIZE, dtype=np.float32)
        sc_host[SC.SC_ALPHA] = sc_host[SC.SC_BALPHA] = args.alpha
        sc_host[SC.SC_RHO_F64:SC.SC_RHO_F64 + 2] = np.array([1.0], dtype=np.float64).view(np.float32)
        sc_host[SC.SC_BRHO_F64:SC.SC_BRHO_F64 + 2] = np.array([1.0], dtype=np.float64).view(np.float32)
        self.sc.copy_(torch.from_numpy(sc_host))
        task.setup()
        self._tickets = torch.zeros(16, dtype=torch.int32, device=dev)     # last-workgroup tickets of the fused launches
        self._ws = {}
        self._noise = None
        self._fit_ws = {}
        self._fit_win_ws = {}                 # fit_node_windows' buffers per (rows, horizon)
        self._val_ws = {}                     # validate_node_windows' own, per (rows, horizon)
        self._val_seed, self._val_gen = int(args.seed), None      # validate_node's private CPU generator (made when needed)
        self._fill = collections.deque()      # pieces of part 1 not yet queued (see _upd_part1)
        self._fill_first = True               # the next solver wait is the first of its update
        self._readback = ScalarsReadback(self.sc)
        for sv in self.task.solvers:          # independent launches go in just before a solver waits for a decision
            sv.before_wait = self._fill_one
        self.use_graphs = False  # replay the update as hipGraphs (single GPU; see update_on_device)
        # per-row steps evaluated inside the MLP / solver launches that produce or consume them (nlbac_gauss_head,
        # nlbac_dy_head, nlbac_in_map / nlbac_out_map, results written to pinned memory by the kernels): False (or
        # NLBAC_FOLD=0) runs every step as the launch of its own it was — same numbers, for A/B runs and the tests
        self.fold_launches = os.environ.get("NLBAC_FOLD", "1") != "0"
        self.sums_defer = os.environ.get("NLBAC_SUMS_DEFER", "1") != "0"      # (Plan.heads; both switches are read there)
        self.adjoint = bool(getattr(args, "adjoint", False))
        self.dp = None          # nlbac_amd.parallel.DataParallel when sharded over GPUs
        self._xb = {}

    @property
    def adjoint(self):
        """True: every NODE solve of the update is differentiated by the continuous adjoint (``odeint_adjoint``,
        BASELINE configs[3]) — the rollouts without a parameter adjoint (the policy loss needs d/d action only), the
        NODE fit with it — instead of back-propagating through the solver's steps."""
        return self._adjoint

    @adjoint.setter
    def adjoint(self, on):
        self._adjoint = bool(on)
        for sv in self.task.solvers:
            sv.adjoint = bool(on)

    def _graphs_on(self):
        # (a dopri5 adjoint solve reads its control block on the host: not capturable)
        return self.use_graphs and self.world == 1 and self.task.graph_ok and not (self._adjoint and self.solver == "dopri5")

    @property
    def node_solver(self):
        return self.task.solvers[0]

    @property
    def fit_solver(self):
        return self.task.fit_solver

    # ------------------------------------------------------------ data parallel
    def enable_data_parallel(self, dist, group=None, always_collective=False, step_control="global"):
        """Shard minibatches over the ranks of ``dist`` (one process per GPU).  Every rank then passes its
        own rows to ``update_*``; losses are normalised by the global batch (``args.batch_size`` must be
        the global size) and gradients / constraint sums are all-reduced (nlbac_amd/parallel.py).

        ``step_control`` (dopri5 only): "global" — the squared error norms of every attempted step are all-reduced, so
        all ranks share the step sizes and accept decisions the single-device run over the global batch takes (what the
        parity tests pin; one small collective per norm, inside the solve).  "shard" — every rank controls the steps of
        its own rows: no collective inside a solve, the ranks' solves run free of each other and meet at the gradient
        all-reduces only; the result is the single-device run with ``row_groups = world`` on its solvers (each shard an
        adaptive solve of its own, as if the reference had been handed the shards one by one), not bit-comparable
        with the global-norm run: the two differ by what a change of step size within rtol / atol changes."""
        from ..parallel import DataParallel
        assert step_control in ("global", "shard")
        self.dp = DataParallel(dist, group, always_collective)
        self.dp_step_control = step_control
        for ar in self.arenas:
            self.dp.broadcast_(ar.theta)
        self.ar_c.hard_update_target()
        self.dp.broadcast_(self.sc)
        self.repack_all()
        for sv in self.task.solvers:
            sv.comm = self.dp if step_control == "global" else None
        return self

    @property
    def world(self):
        return self.dp.world if self.dp is not None else 1

    def _exchange_buf(self, name, n):
        if name not in self._xb:
            self._xb[name] = torch.zeros(n, dtype=torch.float32, device=self.device)
        return self._xb[name]

    def _adam(self, arena, lr, n_slabs, extra=None, target=None, tau=-1.0, before_step=None, alpha=None, mirror=None):
        """Adam on a whole arena.  One GPU: slab sum fused into the step.  Data parallel: local slab sum ->
        flat buffer (+ ``extra`` scalars riding along) -> all-reduce -> step on the reduced gradient."""
        s = stream_ptr()
        a = arena
        # one launch: ++step, slab sum, Adam, Polyak targets and the refresh of the nets' MFMA-fragment weight copies
        scat, scat_t = a.scatter_tables()
        scat_t = scat_t.data_ptr() if (scat_t is not None and target is not None and tau >= 0) else None
        # alpha = exp(log_alpha) refreshed by the step itself: (offsets of the log_alpha entries, where alpha goes)
        n_al = len(alpha[0]) if alpha else 0
        al_off = (C.c_long * 2)(*(list(alpha[0]) + [0, 0])[:2]) if alpha else None
        al_dst = (C.c_void_p * 2)(*(list(alpha[1]) + [None, None])[:2]) if alpha else None
        if self.world == 1:
            if before_step is not None:
                before_step(a.grad.data_ptr())
            # mirror: (pinned host block) the step's last workgroup writes the scalars block to (scalars_readback.py)
            _lib.call("nlbac_adam_fused", a.theta.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.grad.data_ptr(),
                      n_slabs, a.n, a.n, a.state.data_ptr(), lr, target, tau, scat.data_ptr(), scat_t, a.scatter_slots,
                      n_al, al_off, al_dst, self.sc.data_ptr() if mirror is not None else None,
                      mirror.data_ptr() if mirror is not None else None, SC.SC_SIZE if mirror is not None else 0, s)
            return
        n_extra = 0 if extra is None else extra.numel()
        xb = self._exchange_buf("g%d" % id(a), a.n + 4)
        _lib.call("nlbac_reduce_slabs", xb.data_ptr(), a.grad.data_ptr(), n_slabs, a.n, a.n, s)
        if n_extra:
            xb[a.n:a.n + n_extra].copy_(extra)
        self.dp.all_reduce_(xb)
        if n_extra:
            extra.copy_(xb[a.n:a.n + n_extra])
        if before_step is not None:
            before_step(xb.data_ptr())
        _lib.call("nlbac_adam_fused", a.theta.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), xb.data_ptr(), 1, a.n, a.n,
                  a.state.data_ptr(), lr, target, tau, scat.data_ptr(), scat_t, a.scatter_slots, n_al, al_off, al_dst, None,
                  None, 0, s)

    # ------------------------------------------------------------------ utils
    def repack_all(self):
        pack(self.h_crit + self.h_pols + self.h_node)
        pack(self.h_crit, target=True)

    def set_noise(self, eps_list):
        """Pre-drawn N(0,1) draws for the next update, reference order:
        [next_obs sample, obs sample, backup sample (, SimulatedCars: second-step sample, second-step
        backup sample)], each (B, n_u)."""
        self._noise = [torch.as_tensor(e, dtype=torch.float32) for e in eps_list]

    def _scalars(self):
        """Host copy of the device scalars (waits for the launch stream)."""
        return self._readback.read()

    @property
    def alpha(self):
        return float(self._scalars()[SC.SC_ALPHA])

    @property
    def backup_alpha(self):
        return float(self._scalars()[SC.SC_BALPHA])

    @property
    def lambda_values(self):
        return [float(x) for x in self._scalars()[SC.SC_LAMBDA:SC.SC_LAMBDA + self.num_constraints]]

    @property
    def backup_lambda_values(self):
        return [float(x) for x in self._scalars()[SC.SC_BLAMBDA:SC.SC_BLAMBDA + self.num_cbfs]]

    @property
    def augmented_term(self):
        return float(self._scalars()[SC.SC_RHO_F64:SC.SC_RHO_F64 + 2].view(np.float64)[0])

    @property
    def backup_augmented_term(self):
        """Pvtol keeps a separate coefficient for the backup controller (P:59, 1033-1034)."""
        return float(self._scalars()[SC.SC_BRHO_F64:SC.SC_BRHO_F64 + 2].view(np.float64)[0])

    def get_control_bounds(self):
        u_min = torch.tensor(self.env.safe_action_space.low).to(self.device)
        u_max = torch.tensor(self.env.safe_action_space.high).to(self.device)
        return u_min, u_max

    # --------------------------------------------------------- action selection
    def _select(self, policy, state, evaluate, warmup):
        if not warmup and np.ndim(state) == 1:
            return policy.act(np.asarray(state, dtype=np.float64), evaluate)      # one observation: the latency path
        state = to_tensor(np.asarray(state, dtype=np.float64), torch.FloatTensor, self.device)
        expand_dim = len(state.shape) == 1
        if expand_dim:
            state = state.unsqueeze(0)
        if warmup:
            action = torch.stack([torch.from_numpy(self.action_space.sample()) for _ in range(state.shape[0])])
        else:
            a, _, mean = policy.sample(state)
            action = mean if evaluate else a
        action = action.detach().cpu().numpy()
        return action[0] if expand_dim else action

    def select_action(self, state, evaluate=False, warmup=False):
        return self._select(self.policy, state, evaluate, warmup)

    def select_action_backup(self, state, evaluate=False, warmup=False):
        if self.backup_policy is None:
            raise AttributeError("this variant has no backup controller")
        return self._select(self.backup_policy, state, evaluate, warmup)

    # ------------------------------------------------------------------ update
    def update_parameters(self, memory, batch_size, updates, dynamics_model, NODE_memory, NODE_model_update_interval,
                          i_episode=None):
        """Same contract as the reference (sac_cbf_clf.py:181-319): one sampled
        minibatch -> 6 floats.  ``dynamics_model`` is accepted for signature
        parity; obs->state runs on the device.  ``i_episode`` is the Pvtol copy's trailing argument (P:181):
        its NODE fit stops after episode 100 (P:205)."""
        fit = updates % NODE_model_update_interval == 0 and self.task.fit_due(i_episode)
        # (sac_cbf_clf.py:205: min(NODE_memory.position, 32768).  ``position`` wraps with the ring: a replay that has just
        #  wrapped reports 0 — the reference would then sample zero rows and fail — and the fit takes the filled size)
        nb = min(NODE_memory.position or len(NODE_memory), 32768) if fit else 0
        fit = fit and nb > 0
        if fit and self.node_horizon > 1:            # multi-step fit on trajectory windows (same draw order: below)
            return self._update_with_window_fit(memory, batch_size, updates, NODE_memory, nb)
        if hasattr(memory, "sample_rows"):           # replay resident in HBM: gather on the device
            ws = self._workspace(batch_size)
            eps_ready = self._noise is None and getattr(memory, "device_rng", False)
            memory.sample_rows(batch_size, out=ws.mb, **({"eps_out": ws.eps} if eps_ready else {}))
            if fit:                                  # same draw order as the reference: minibatch, then NODE rows
                self.fit_node_rows(NODE_memory.sample_rows(nb) if hasattr(NODE_memory, "sample_rows") else
                                   self._rows_from_host(NODE_memory.sample(batch_size=nb)).to(self.device))
            return self.update_on_device(ws, updates, eps_ready=eps_ready)
        batch = memory.sample(batch_size=batch_size)
        node_rows = NODE_memory.sample(batch_size=nb) if fit else None
        return self.update_from_host(batch, updates, node_rows)

    def _rows_from_host(self, batch):
        """Pack the 10-tuple of ``ReplayMemory.sample`` into minibatch-layout rows (one H2D copy)."""
        lay = self.lay
        batch = tuple(batch)
        sig = None
        if lay.sig is not None:        # 11 fields: barrier_signal sits after the constraint
            sig, batch = batch[4], batch[:4] + batch[5:]
        state, action, reward, constraint, lya_in, next_lya_in, nstate, mask = batch[:8]
        n = np.asarray(state).shape[0]
        host = np.zeros((n, lay.LD), dtype=np.float32)
        if sig is not None:
            host[:, lay.sig] = sig
        host[:, lay.obs:lay.obs + lay.obs_dim] = state
        host[:, lay.act:lay.act + lay.act_dim] = np.asarray(action).reshape(n, lay.act_dim)
        host[:, lay.rew], host[:, lay.con] = reward, constraint
        host[:, lay.lya:lay.lya + lay.lya_dim] = lya_in
        host[:, lay.nlya:lay.nlya + lay.lya_dim] = next_lya_in
        host[:, lay.nobs:lay.nobs + lay.obs_dim] = nstate
        host[:, lay.mask] = mask
        if len(batch) > 9 and batch[8] is not None and np.asarray(batch[8]).dtype != object:
            host[:, lay.t], host[:, lay.nt] = batch[8], batch[9]
        return torch.from_numpy(host)

    def update_from_host(self, batch, updates, node_batch=None):
        """batch / node_batch: tuples of numpy arrays in the field order of ``ReplayMemory.sample``
        (node_batch may also be the short form (obs, action, next_obs[, t]))."""
        B = np.asarray(batch[0]).shape[0]
        ws = self._workspace(B)
        ws.mb.copy_(self._rows_from_host(batch), non_blocking=False)
        if node_batch is not None:
            if len(node_batch) <= 4:       # (obs, action, next_obs[, t]) -> full field order
                o, a_, no = node_batch[:3]
                n = np.asarray(o).shape[0]
                t = np.asarray(node_batch[3]).reshape(n) if len(node_batch) == 4 else np.zeros(n)
                zl = np.zeros((n, self.lay.lya_dim))
                node_batch = (o, a_, np.zeros(n), np.zeros(n)) + ((np.zeros(n),) if self.lay.sig is not None else ()) \
                    + (zl, zl, no, np.ones(n), t, t)
            self.fit_node_rows(self._rows_from_host(node_batch).to(self.device))
        return self.update_on_device(ws, updates)

    def _workspace(self, B):
        if B not in self._ws:
            self._ws[B] = _Workspace(B, self.hidden, self.device, self.lay, self.task)
        return self._ws[B]

    # -- NODE fit (model.py:221-260 via sac_cbf_clf.py:205-219) -----------------
    def fit_node_rows(self, rows):
        """One Adam step of the NODE regression on a device tensor of minibatch-layout rows (N, LD)
        (obs, action, next_obs and, where the model takes it, t are read in place)."""
        self._fit(*self.task.fit_inputs(rows))

    def _fit(self, p_obs, obs_ld, action, p_nobs, nobs_ld, N):
        task = self.task
        self._fill.clear()      # (pieces of an update that raised half-way must not run behind this fit's solves)
        if N not in self._fit_ws:
            while len(self._fit_ws) >= 2:       # the fit batch grows with the replay: keep the two latest sizes only
                self._fit_ws.pop(next(iter(self._fit_ws)))      # (its graphs go with it)
            w = task.fit_ws(N)
            w.update(graphs=GraphCache(task.solvers), warm=0)
            self._fit_ws[N] = w
        w = self._fit_ws[N]
        w["u"].copy_(action)
        key = (p_obs, obs_ld, p_nobs, nobs_ld, self.solver)
        part1 = lambda: task.fit_part1(w, p_obs, obs_ld, p_nobs, nobs_ld, N)
        if not self._graphs_on() or w["warm"] < 1:
            w["warm"] += 1
            part1()
            self._fit_part2(w, N, task.fit_solver.forward_finish())
            return
        g = w["graphs"]
        g.replay(("p1",) + key, part1)
        if self.solver == "dopri5" and not task.fit_solver.first_step_done():
            self._fit_part2(w, N, task.fit_solver.forward_finish())      # rare: finish this one eagerly
            return
        g.replay(("p2",) + key, lambda: self._fit_part2(w, N, task.fit_solver.forward_finish(assume_single_step=True)))

    def _fit_part2(self, w, N, pred):
        s = stream_ptr()
        ns = self.task.n_s
        nblk = (N + 255) // 256
        NG = N * self.world
        _lib.call("nlbac_mse_fwd_bwd", pred.data_ptr(), ns, w["nst"].data_ptr(), ns, N, NG, ns, w["dpred"].data_ptr(),
                  ns, w["part"].data_ptr(), s)
        _lib.call("nlbac_sum_partials", w["part"].data_ptr(), nblk, 1, 1.0 / (NG * ns),
                  self.sc.data_ptr() + 4 * SC.SC_NODE_LOSS, s)
        self.task.fit_solver.backward(w["dpred"], need_du=False, need_params=True)
        # every accepted RK step writes its own gradient slabs; a solve with many steps takes narrower ones
        n_steps = max(1, len(self.task.fit_solver.ctx.get("steps") or [None]))
        used = self.task.fit_solver.accumulate_param_grads(
            self.ar_n, max(1, min(self.n_fit_slabs, self.ar_n.n_slabs // min(n_steps, self.ar_n.n_slabs))))
        self._adam(self.ar_n, 1e-3, used, extra=self.sc[SC.SC_NODE_LOSS:SC.SC_NODE_LOSS + 1])

    # -- multi-step NODE fit on trajectory windows (node_horizon > 1) ------------------------
    def _update_with_window_fit(self, memory, batch_size, updates, NODE_memory, nb):
        """``update_parameters`` when a multi-step fit is due: minibatch draw, window draw (the reference's order:
        minibatch first, then the NODE rows), the fit, the update."""
        H, stride = self.node_horizon, self.node_stride
        on_device = hasattr(memory, "sample_rows")
        if on_device:
            ws = self._workspace(batch_size)
            eps_ready = self._noise is None and getattr(memory, "device_rng", False)
            memory.sample_rows(batch_size, out=ws.mb, **({"eps_out": ws.eps} if eps_ready else {}))
        else:
            batch = memory.sample(batch_size=batch_size)
        if (H - 1) * stride < len(NODE_memory):      # (a replay shorter than one window: nothing to fit on yet)
            if hasattr(NODE_memory, "sample_windows") and hasattr(NODE_memory, "sample_rows"):
                rows, valid = NODE_memory.sample_windows(nb, H, stride)
                self.fit_node_windows(rows, valid, NODE_memory.window_counts)
            else:                                    # host replay: its own rule, packed step by step
                fields, valid = NODE_memory.sample_windows(nb, H, stride)
                rows = torch.stack([self._rows_from_host(tuple(f[k] for f in fields)) for k in range(H)])
                self.fit_node_windows(rows.to(self.device), torch.from_numpy(valid.astype(np.float32)))
        if on_device:
            return self.update_on_device(ws, updates, eps_ready=eps_ready)
        return self.update_from_host(batch, updates, None)

    def fit_node_windows(self, rows, valid=None, counts=None):
        """One Adam step of the NODE regression over trajectory windows: ``rows`` (H, N, LD) minibatch-layout rows on
        the device, step k of window i at ``rows[k, i]`` (``DeviceReplayMemory.sample_windows``); ``valid`` (N,): windows
        with 0 do not count (None: all do); ``counts``: the int32 sums of ``valid`` per 256 windows where the caller has
        them (``DeviceReplayMemory.window_counts``), else formed here.

        x_0 = state(obs of step 0), target_k = state(next_obs of step k), the carried columns of step k as ``fit_inputs``
        forms them; the H intervals are ONE solve (``ode_traj.solve``: one launch forward, one backward and one
        weight-gradient pass for euler / rk4, chained interval by interval for dopri5), the loss ``nlbac_traj_mse_fwd_bwd``
        (masked MSE, normalised by valid windows x H x n_s) lands in the scalars block where the one-step fit leaves
        its own, and the agent's Adam kernel steps the NODE arena.  Runs eagerly (never captured into a hipGraph)."""
        from .. import ode_traj as T
        from ..rollout import _one_launch_ok
        if self.world > 1:
            raise RuntimeError("fit_node_windows: trajectory windows are not sharded over GPUs; use node_horizon = 1 "
                               "under enable_data_parallel")
        if rows.dim() != 3 or rows.shape[2] != self.lay.LD or rows.dtype != torch.float32 or not rows.is_cuda:
            raise ValueError("fit_node_windows: rows must be a float32 device tensor (H, N, %d); got %s"
                             % (self.lay.LD, tuple(rows.shape)))
        rows = rows.contiguous()
        H, N, LD = rows.shape
        task, lay, model, ns = self.task, self.lay, self.neural_ode_model, self.task.n_s
        self._fill.clear()      # (as _fit: pieces of an update that raised half-way must not run behind this fit)
        w = self._fit_windows_ws(N, H)
        if valid is not None and counts is None:
            valid, counts = valid_counts(valid, N, self.device)
        elif valid is not None:
            valid = valid.to(self.device, torch.float32).contiguous()
            assert valid.numel() == N and counts.numel() == (N + 255) // 256 and counts.dtype == torch.int32
        # every step's rows as one (H N, LD) block: the task's hooks read them in place
        flat = rows.view(H * N, LD)
        p_obs, obs_ld, ctl, p_nobs, nobs_ld, _ = task.fit_inputs(flat)
        task.state_rows(p_obs, obs_ld, N, w["x0"])                      # step 0's observation
        task.state_rows(p_nobs, nobs_ld, H * N, w["target"])            # every step's next observation
        w["u"].view(H * N, -1).copy_(ctl)                               # every step's carried columns
        dt = float(torch.tensor([0.0, float(self.env.dt)], dtype=torch.float32)[1])      # (as odeint's time grid rounds it)
        kept = T.solve(model, T.EqualSteps(dt, H), self.solver, "params", _one_launch_ok(model, self.solver),
                       w["x0"], w["u"], w["xs"], self.atol, self.rtol)
        dout = w["dout"]                                                # (H + 1, N, n_s); dout[0] stays zero
        traj_mse_launch(w["xs"], w["target"], valid, counts, H, N, ns, dout[1:], w["part"],
                        self.sc.data_ptr() + 4 * SC.SC_NODE_LOSS)
        _, _, flat_grad = kept.backward(dout, need_p=True)
        a = self.ar_n
        used = a.n_slabs                  # one launch: the weight-gradient pass left its slab partials in the arena
        if isinstance(kept, T.Chain):     # chained: every interval reduced its own slabs; their sum goes in as slab 0
            a.grad[0].copy_(flat_grad)
            used = 1
        self._adam(a, 1e-3, used, extra=self.sc[SC.SC_NODE_LOSS:SC.SC_NODE_LOSS + 1])

    def _fit_windows_ws(self, N, H):
        if (N, H) not in self._fit_win_ws:
            while len(self._fit_win_ws) >= 2:       # as _fit_ws: the fit batch grows with the replay
                self._fit_win_ws.pop(next(iter(self._fit_win_ws)))
            z, ns = self.task.z, self.task.n_s
            nc = self.neural_ode_model.n_u if self.neural_ode_model.affine else self.neural_ode_model.n_carry
            self._fit_win_ws[(N, H)] = dict(x0=z(N, ns), target=z(H, N, ns), u=z(H, N, nc), xs=z(H, N, ns),
                                            dout=z(H + 1, N, ns), part=z(loss_blocks(H, N, ns)))
        return self._fit_win_ws[(N, H)]

    # -- NODE validation over trajectory windows ---------------------------------------------
    def validate_node_windows(self, rows, valid=None, counts=None):
        """The NODE's prediction error over trajectory windows, by look-ahead step and state component:
        ``fit_node_windows`` up to the loss — the same ``rows`` (H, N, LD) / ``valid`` / ``counts`` contract (``counts``
        is accepted and not needed), ``fit_inputs``, ``state_rows`` for x_0 and the targets, the carried columns, ``dt``
        on the float32 grid, ONE ``ode_traj.solve`` over the H intervals that keeps nothing — then
        ``nlbac_traj_err_stats`` instead of the loss.  Returns ``(stats (5, H, n_s) float64, nvalid () int64)`` on the
        device without a synchronisation (``node_fit.error_report`` reads them).

        Measures only: the scalars block (``SC_NODE_LOSS`` keeps the last fit's value), the arenas, Adam's state, every
        generator, the fit's workspaces and the update's queued pieces stay as they are; its buffers are its own, two
        shapes at most.  Angles are not wrapped (``node_fit.validate_rollout``)."""
        from .. import ode_traj as T
        from ..node_fit import traj_error_stats_launch
        from ..rollout import _one_launch_ok
        if self.world > 1:
            raise RuntimeError("validate_node_windows: trajectory windows are not sharded over GPUs; use node_horizon = 1 "
                               "under enable_data_parallel")
        if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or rows.shape[2] != self.lay.LD \
                or rows.dtype != torch.float32 or not rows.is_cuda:
            raise ValueError("validate_node_windows: rows must be a float32 device tensor (H, N, %d); got %s"
                             % (self.lay.LD, tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__))
        rows = rows.contiguous()
        H, N, LD = rows.shape
        task, model, ns = self.task, self.neural_ode_model, self.task.n_s
        if valid is not None:
            valid = (torch.as_tensor(valid).to(self.device).reshape(-1) != 0).to(torch.float32).contiguous()
            if valid.numel() != N:
                raise ValueError("validate_node_windows: valid must hold one entry per window (%d); got %d"
                                 % (N, valid.numel()))
        w = self._validate_ws(N, H)
        flat = rows.view(H * N, LD)
        p_obs, obs_ld, ctl, p_nobs, nobs_ld, _ = task.fit_inputs(flat)
        task.state_rows(p_obs, obs_ld, N, w["x0"])                      # step 0's observation
        task.state_rows(p_nobs, nobs_ld, H * N, w["target"])            # every step's next observation
        w["u"].view(H * N, -1).copy_(ctl)                               # every step's carried columns
        dt = float(torch.tensor([0.0, float(self.env.dt)], dtype=torch.float32)[1])      # (as odeint's time grid rounds it)
        T.solve(model, T.EqualSteps(dt, H), self.solver, "none", _one_launch_ok(model, self.solver),
                w["x0"], w["u"], w["xs"], self.atol, self.rtol)
        stats = torch.empty(5, H, ns, dtype=torch.float64, device=self.device)      # (the caller's: a driver keeps a list)
        nvalid = torch.empty((), dtype=torch.int64, device=self.device)
        traj_error_stats_launch(w["xs"], w["target"], w["x0"], valid, H, N, ns, w["scratch"], stats, nvalid)
        return stats, nvalid

    def _validate_ws(self, N, H):
        ws = self._val_ws
        if (N, H) not in ws:
            from ..node_fit import stats_scratch_doubles
            while len(ws) >= 2:                    # as _fit_win_ws
                ws.pop(next(iter(ws)))
            z, ns = self.task.z, self.task.n_s
            nc = self.neural_ode_model.n_u if self.neural_ode_model.affine else self.neural_ode_model.n_carry
            ws[(N, H)] = dict(x0=z(N, ns), target=z(H, N, ns), u=z(H, N, nc), xs=z(H, N, ns),
                              scratch=torch.empty(stats_scratch_doubles(H, N, ns), dtype=torch.float64, device=self.device))
        return ws[(N, H)]

    VALIDATE_SEED_TAG = 0x6E6F64655F76616C      # the private generator of validate_node: args.seed and this tag

    def validate_node(self, memory, n_windows, horizon=None, stride=None, idx=None, generator=None):
        """``validate_node_windows`` on ``n_windows`` windows of ``horizon`` steps ``stride`` rows apart out of the replay
        ``memory`` (defaults: the agent's ``node_horizon`` / ``node_stride``).  Start rows: ``idx`` (int64, one per
        window), else ``torch.randint(0, len(memory), (n_windows,), generator=g)`` with ``g`` = ``generator`` or a CPU
        generator of the agent's own, seeded from ``args.seed`` and a fixed tag when first needed; the replay's gather
        launch decides which windows are unbroken trajectories (``nlbac_gather_windows``; a host ``ReplayMemory`` applies
        the same rule and is packed step by step).  Returns ``(stats, nvalid)`` on the device, or None while
        ``(horizon - 1) * stride >= len(memory)`` — nothing to validate on yet.

        Leaves as found: the replay's draw counter and ``window_counts``, Python's ``random``, numpy's global generator,
        torch's global CPU and CUDA generators — a training run that validates in between continues bit for bit."""
        H = self.node_horizon if horizon is None else horizon
        stride = self.node_stride if stride is None else stride
        for name, v in (("n_windows", n_windows), ("horizon", H), ("stride", stride)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("validate_node: %s must be an integer >= 1; got %r" % (name, v))
        if generator is not None and (not isinstance(generator, torch.Generator) or generator.device.type != "cpu"):
            raise ValueError("validate_node: generator must be a CPU torch.Generator")
        if idx is not None:
            idx = torch.as_tensor(idx)
            if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() != n_windows:
                raise ValueError("validate_node: idx must be %d int64 start rows" % n_windows)
        if self.world > 1:
            raise RuntimeError("validate_node: trajectory windows are not sharded over GPUs; use node_horizon = 1 "
                               "under enable_data_parallel")
        H, stride, n_windows = int(H), int(stride), int(n_windows)
        if (H - 1) * stride >= len(memory):
            return None
        if idx is None:
            g = generator
            if g is None:
                g = self._val_gen
                if g is None:
                    g = self._val_gen = torch.Generator()
                    g.manual_seed((self._val_seed * 0x9E3779B97F4A7C15 + self.VALIDATE_SEED_TAG) & 0x7FFFFFFFFFFFFFFF)
            idx = torch.randint(0, len(memory), (n_windows,), generator=g, dtype=torch.int64)
        if hasattr(memory, "sample_rows") and hasattr(memory, "sample_windows"):
            had, counts = hasattr(memory, "window_counts"), getattr(memory, "window_counts", None)
            draws = getattr(memory, "_draws", None)      # (a replay without a draw counter has none to put back)
            try:
                rows, valid = memory.sample_windows(n_windows, H, stride, idx=idx)
            finally:
                if draws is not None:
                    memory._draws = draws
                if had:
                    memory.window_counts = counts
                elif hasattr(memory, "window_counts"):
                    del memory.window_counts
        else:                                        # host replay: its own rule, packed step by step
            fields, valid = memory.windows_at(idx.numpy(), H, stride)
            rows = torch.stack([self._rows_from_host(tuple(f[k] for f in fields)) for k in range(H)]).to(self.device)
            valid = torch.from_numpy(valid.astype(np.float32))
        return self.validate_node_windows(rows, valid)

    # -- the update proper --------------------------------------------------------
    def _plan(self, ws, NP=None):
        """The launch arguments of ``ws`` for an update of ``NP`` controllers (update_plan.Plan), built once."""
        NP = NP or self.task.n_pol
        return ws.plan.get(NP) or ws.plan.setdefault(NP, Plan(self, ws, NP))

    def auglag_fused(self, ws, P, lam_upd):
        """The (fused, ticket, sc) tail of a ``*_constraints_fwd`` call: on one GPU the launch's last workgroup runs the
        augmented-Lagrangian step (``nlbac_auglag``) itself; under data parallelism the sums are all-reduced first.
        Per update: the two lambda-update flags of the plan's ``nlbac_auglag_args``."""
        if self.world > 1:
            return None, None, None
        P.auglag.do_lambda_update, P.auglag.do_backup_lambda_update = lam_upd, ws.blam_upd
        return C.byref(P.auglag), self._tickets.data_ptr() + 4 * 12, self.sc.data_ptr()

    def auglag(self, ws, n_cbf, lam_upd):
        """required_matrix, ratio, lambda / rho updates and loss coefficients from the constraint partial sums
        (all-reduced first under data parallelism: they enter the loss nonlinearly).  Single GPU: already done by the
        constraints launch (``auglag_fused``)."""
        s, call = stream_ptr(), _lib.call
        NP = ws.np_now
        if self.world == 1:
            ws.p_part_q, ws.n_part_q = ws.part_q.data_ptr(), ws.nblk
            return
        ncol = n_cbf + 1 + (n_cbf if NP == 2 else 0)
        xs = self._exchange_buf("sums", 64)
        call("nlbac_sum_partials", ws.part_c.data_ptr(), ws.nblk, ncol, 1.0, xs.data_ptr(), s)
        for pp in range(NP):
            call("nlbac_sum_partials", ws.part_q[pp].data_ptr(), ws.nblk, 2, 1.0, xs.data_ptr() + 4 * (32 + 2 * pp), s)
        self.dp.all_reduce_(xs)
        ws.p_part_q, ws.n_part_q = xs.data_ptr() + 4 * 32, 1
        call("nlbac_auglag", xs.data_ptr(), 1, n_cbf, 1, float(self.batch_size), lam_upd, ws.blam_upd,
             self.task.ratio_mode, self.task.backup_mode if NP == 2 else 0, self.task.lam_lo, self.task.lam_hi,
             self.sc.data_ptr(), s)

    def update_on_device(self, ws, updates, sync=True, eps_ready=False, prefetch=None):
        """Minibatch already in ``ws.mb``; returns the reference's 6 floats.  ``eps_ready``: ``ws.eps`` already holds
        this update's N(0,1) draws (``DeviceReplayMemory.sample_rows(..., eps_out=ws.eps)``).

        ``prefetch``: a callable that draws a minibatch into ``ws.mb`` / ``ws.eps`` with device launches only
        (``lambda: replay.sample_rows(B, out=ws.mb, eps_out=ws.eps)``); the caller then never draws itself.  This update's
        rows are drawn by it unless the previous call already has: behind its last launch (the actors' optimiser step —
        nothing reads ``ws.mb`` after it) every update queues the NEXT update's draw and policy forward before the host
        blocks on the six returned floats, so the update boundary — the host waking up, returning to its loop and coming
        back with the first launches, ~30 us of idle GPU otherwise — is covered by ~30 us of queued work.  The draw sees
        the replay as of the end of this update: a driver that pushes transitions between two updates and wants them
        eligible at once does not pass ``prefetch``."""
        pre, ws._prefetched = ws._prefetched, None
        if prefetch is not None:
            eps_ready = True
            if pre is None or pre[0] != updates:
                pre = None
                prefetch()
        else:
            pre = None
        ws._pre_now, ws._prefetch_fn, ws._sync = pre, prefetch, sync
        if self._noise is not None:
            assert len(self._noise) == self.task.n_eps, "set_noise needs %d draws" % self.task.n_eps
            order = self.task.eps_order or range(self.task.n_eps)     # device slot -> reference draw index
            for i, j in enumerate(order):
                ws.eps[i].copy_(self._noise[j].to(self.device).reshape(ws.eps[i].shape))
            self._noise = None
        elif not eps_ready:
            ws.eps.normal_()
        soft = (updates % self.target_update_interval == 0)
        lam_upd = 1 if updates % self.Lagrangian_multiplier_update_interval == 0 else 0
        NP = ws.np_now = self.task.n_pol_now(updates)
        ws.updates_now = updates
        assert ws._pre_now is None or ws._pre_now[1] == NP
        ws.blam_upd = self.task.backup_lam_due(updates, self.Lagrangian_multiplier_update_interval)
        self._readback.choose_mirror(sync, self.world == 1 and not self._graphs_on() and self.fold_launches)
        if not self._graphs_on() or ws.warm < 1:
            ws.warm += 1
            self._upd_part1(ws, soft)
            self._upd_part2(ws, lam_upd, False)
        else:
            # hipGraph replay: part 1 up to the dopri5 accept decision, one 256-byte read, part 2
            g = ws.graphs
            k1, k2 = ("p1", soft, self.solver, NP), ("p2", lam_upd, ws.blam_upd, self.solver, NP)
            g.replay(k1, lambda: self._upd_part1(ws, soft))
            if self.solver == "dopri5" and not self.task.first_step_done():
                self._upd_part2(ws, lam_upd, False)          # rare: finish eagerly
            else:
                g.replay(k2, lambda: self._upd_part2(ws, lam_upd, True))
        h = self._readback.returns(sync)      # (sync False, or the first "lagged" call: None)
        if h is None:
            return None
        alpha_loss = float(h[SC.SC_ALOSS]) if self.automatic_entropy_tuning else 0.0
        return (float(h[SC.SC_QF1]), float(h[SC.SC_QF2]), float(h[SC.SC_LF]), float(h[SC.SC_PL1]),
                alpha_loss, float(h[SC.SC_ALPHA]))

    def _upd_part1(self, ws, soft):
        """Phases A, B and the forward half of C up to the rollout's first host decision point."""
        B, A = ws.B, self.lay.act_dim
        G = B * self.world                      # rows the batch means run over
        s = stream_ptr()
        NP = ws.np_now
        P = self._plan(ws, NP)
        LD = P.LD

        # ---- A. targets (no grad): pi(s'), Q_target(s', a'), L_target(c') ; critic / Lyapunov forward
        if ws._pre_now is None:       # (else: queued behind the previous update's last launch, see prefetch)
            self._policy_forward(ws, P, NP)
        # the rollout of the learned dynamics needs only pi(s) and the NODE: its first attempted step goes in here,
        # so that the critic phase below is queued behind it while the host waits for the accept decision
        self.task.rollout_begin(ws, P)
        # The rest of part 1 does not depend on the rollout.  It is cut into three pieces that the solvers pull in one
        # at a time just before each wait for an accept decision (``before_wait``), so that every attempted step —
        # the second of a two-step solve, the second and third solve of Pvtol's chain — has work queued behind it;
        # whatever is left goes in when the rollout is finished (``drain_fill``, called by the task).
        self._fill = collections.deque((lambda: self._part1_targets(ws, P, B, G, LD, s),
                                        lambda: self._part1_critic_step(ws, P, B, soft),
                                        lambda: self._part1_actor_q(ws, P, B, G, NP, s)))
        # how many pieces the first wait pulls: a rollout of ONE adaptive solve gets them all at once (the host needs
        # ~100 us of queued work to read the decision and come back); chained solves (SimulatedCars 2, Pvtol 3) one per wait
        self._fill_first = self.task.rollout_waits == 1
        if ws._pre_now is not None and ws._pre_now[2]:
            self._fill.popleft()                # (targets + critic data backward: queued with the prefetch)
            # (the first wait still queues both remaining pieces: holding the Q(s, pi) forward back for the launch it
            #  could share with V(p(x')) left the stream dry for ~20 us while the host got from the accept decision to
            #  that launch)
        if self.solver != "dopri5" or torch.cuda.is_current_stream_capturing():
            self.drain_fill()                   # no waits on this path (fixed-step solver / graph capture)

    def _policy_forward(self, ws, P, NP):
        """pi(s') and the actors on s.  (The actors' forward on s does not depend on the critic step: it shares pi(s')'s
        launch, and all (1+NP)*B samples are drawn by one launch - eps[0 .. NP] are contiguous.)"""
        B, A = ws.B, self.lay.act_dim
        s, call = stream_ptr(), _lib.call
        if self.fold_launches:      # (the samples are drawn by the policy launch itself: nlbac_gauss_head)
            assert P.head_pol3 is not None
            call("nlbac_mlp_fwd_gauss", P.n_pol3, P.io_pol3, 1 + NP, B, C.byref(P.head_pol3), s)
        else:
            pol = self.policy
            call("nlbac_mlp_fwd", P.n_pol3, P.io_pol3, 1 + NP, B, s)
            call("nlbac_gauss_sample_fwd", ws.heads3.data_ptr(), 2 * A, ws.eps.data_ptr(), pol.action_scale.data_ptr(),
                 pol.action_bias.data_ptr(), A, (1 + NP) * B, ws.act3.data_ptr(), A, ws.logp3.data_ptr(), s)

    def _prefetch_next(self, ws, updates):
        """Behind this update's last launch: the next update's minibatch draw and first launches (update_on_device)."""
        fn = ws._prefetch_fn
        if fn is None or self._graphs_on() or self.world != 1 or self._noise is not None:
            return
        if ws._sync and self._readback.mirror is None:
            return      # (the returned floats would be copied BEHIND the queued launches, whose dy head rewrites the losses)
        fn()
        NP = self.task.n_pol_now(updates + 1)
        ws._prefetched = (updates + 1, NP, self._prefetch_launches(ws, NP))

    def update_prefetch(self, ws, updates, prefetch):
        """Draw update ``updates``'s minibatch (``prefetch``, see update_on_device) and queue its policy forward now — what
        every update does for its successor; for callers that need the draw to come before something else they queue."""
        if self._graphs_on() or self.world != 1:
            return
        prefetch()
        NP = self.task.n_pol_now(updates)
        ws._prefetched = (updates, NP, self._prefetch_launches(ws, NP))

    def _prefetch_launches(self, ws, NP):
        """What of an update needs nothing but its minibatch and the parameters as the previous update left them: the
        policy forward, then the target / critic forward and the critics' data backward (~95 us of launches: more than
        the host needs to come round to the next update)."""
        P = self._plan(ws, NP)
        self._policy_forward(ws, P, NP)
        # (a rollout of three chained solves keeps the targets piece for its waits: each solve's accept decision is a
        #  host round trip, and a piece of independent work queued behind every one of them is worth more than a longer
        #  head start — the policy forward alone covers the update boundary at those batch sizes.  Returns whether the
        #  targets piece went out.)
        if self.task.rollout_waits >= 3:
            return False
        self._part1_targets(ws, P, ws.B, ws.B * self.world, P.LD, stream_ptr())
        return True

    def _fill_one(self):
        """Called by a solver just before it waits for an accept decision: queue the next piece(s) of part 1 behind the
        attempted step.  The first wait of an update gets two (the host needs ~100 us of queued work to read the
        decision and launch what follows without the stream running dry), later ones one each."""
        k, self._fill_first = (2 if self._fill_first else 1), False
        while k and self._fill:
            self._fill.popleft()()
            k -= 1

    def drain_fill(self):
        while self._fill:
            self._fill.popleft()()

    def _part1_targets(self, ws, P, B, G, LD, s):
        sc, call = self.sc.data_ptr(), _lib.call
        one = self.world == 1
        call("nlbac_mlp_fwd", P.n_six, P.io_six, P.n_six_count, B, s)
        q = ws.q6
        if one and len(self.h_extra) <= 1 and self.fold_launches:
            # single GPU, no extra critic: targets, dL/dq and the three losses are produced by the critics' data backward
            # itself (nlbac_dy_head kind 2) — no launch between the six-net forward and the backward
            assert P.head_td is not None
            call("nlbac_mlp_bwd_data_head", P.n_crit, P.io_crit, len(self.h_crit), B, C.byref(P.head_td), s)
            return
        call("nlbac_td_targets", q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), ws.nlogp.data_ptr(),
             P.p_rew, P.p_con, P.p_mask, LD, q[3].data_ptr(), q[4].data_ptr(), q[5].data_ptr(),
             sc + 4 * SC.SC_ALPHA, self.gamma, B, G, ws.dq3[0].data_ptr(), ws.dq3[1].data_ptr(), ws.dq3[2].data_ptr(),
             ws.next_q.data_ptr(), ws.next_l.data_ptr(), ws.part_td.data_ptr(),
             *((self._tickets.data_ptr(), 1.0 / G, sc + 4 * SC.SC_QF1) if one else (None, 0.0, None)), s)
        if not one:       # (single GPU: the launch's last workgroup has summed the three losses itself)
            call("nlbac_sum_partials", ws.part_td.data_ptr(), ws.nblk, 3, 1.0 / G, sc + 4 * SC.SC_QF1, s)
        for k in range(len(self.h_extra)):      # barrier TD step (NU/sac_cbf_clf.py:224-233)
            call("nlbac_td_value", q[6 + 2 * k].data_ptr(), ws.mb.data_ptr() + 4 * self.lay.sig, LD, P.p_mask, LD,
                 q[7 + 2 * k].data_ptr(), self.gamma, B, G, ws.dq3[3 + k].data_ptr(), None, ws.part_tdx[k].data_ptr(),
                 *((self._tickets.data_ptr() + 4 * (1 + k), 1.0 / G, sc + 4 * SC.SC_XLOSS) if one else (None, 0.0, None)), s)
            if not one:
                call("nlbac_sum_partials", ws.part_tdx[k].data_ptr(), ws.nblk, 1, 1.0 / G, sc + 4 * SC.SC_XLOSS, s)

        # ---- B. critic / Lyapunov backward + Adam (+ Polyak targets) ---------------
        call("nlbac_mlp_bwd_data", P.n_crit, P.io_crit, len(self.h_crit), B, s)

    def _part1_critic_step(self, ws, P, B, soft):
        a = self.ar_c
        bwd_weights(P.n_crit, P.io_crit, len(self.h_crit), B, a.n_slabs, a.n, self.device, ws=P.sk_crit)
        self._adam(a, self.critic_lyapunov_lr, a.n_slabs, extra=self.sc[SC.SC_QF1:SC.SC_QF1 + 3],
                   target=a.target.data_ptr(), tau=self.tau if soft else -1.0)

    def _part1_actor_q(self, ws, P, B, G, NP, s):
        # ---- C. actors: Q(s, pi) with the stepped critics (the rollout was started in phase A) -----
        sc, call = self.sc.data_ptr(), _lib.call
        call("nlbac_mlp_fwd", P.n_q5, P.io_q5, P.n_q5_count, B, s)
        if self.world == 1 and self.fold_launches:
            return               # (the branch terms and their sums come out of the Q(s, pi) data backward: P.head_actor_q)
        fused = ticket = None
        if self.world == 1:      # policy_loss_1 / alpha losses / d log_alpha by the launch's last workgroup (nlbac_actor_scalars)
            assert P.actor_scalars is not None
            fused, ticket = C.byref(P.actor_scalars), self._tickets.data_ptr() + 4 * 8
        call("nlbac_actor_q_terms", ws.qpi[0].data_ptr(), ws.qpi[1].data_ptr(), ws.logp2.data_ptr(),
             sc + 4 * SC.SC_ALPHA, B, G, NP, ws.dq_pi[0].data_ptr(), ws.dq_pi[1].data_ptr(), ws.part_q.data_ptr(), fused, ticket, s)

    def _upd_part2(self, ws, lam_upd, assume_single):
        """Constraints, augmented-Lagrangian scalars, the whole actor backward and the actor Adam step."""
        B, A, Do = ws.B, self.lay.act_dim, self.lay.obs_dim
        G = B * self.world
        s = stream_ptr()
        NP = ws.np_now
        P = self._plan(ws, NP)
        sc, call = self.sc.data_ptr(), _lib.call
        ws.q5_bwd_done = False       # (a task may run the Q(s, pi) data backward inside one of its own launches)
        du2, du_ld = self.task.loss_and_backward(ws, P, lam_upd, assume_single)

        # the Q(s, pi) nets (dx only): single GPU — d min(Q1, Q2), policy_loss_1, the alpha losses and d log_alpha are
        # produced by this launch (nlbac_dy_head kind 3); data parallel — nlbac_actor_q_terms ran in part 1
        if ws.q5_bwd_done:
            pass
        elif self.world == 1 and self.fold_launches:
            assert P.head_actor_q is not None
            call("nlbac_mlp_bwd_data_head", P.n_q5, P.io_q5, 2 * NP, B, C.byref(P.head_actor_q), s)
        else:
            call("nlbac_mlp_bwd_data", P.n_q5, P.io_q5, 2 * NP, B, s)
        # the actors: d heads from d action (two Q nets + the rollout) and d logp, inside their data backward (kind 1)
        if self.fold_launches:
            H = P.head_gauss
            assert H is not None
            # per update: the rollout's d action, and the augmented-Lagrangian step a constraint head deferred (tasks.py:
            # cf_job; its lambda-update flags change from update to update), which this launch commits
            H.da[2], H.da_ld[2] = du2.data_ptr(), du_ld
            job = P.cf_job
            F = H.finish[2]
            F.kind = 4 if job else 0
            if job:
                F.partials, F.sc = job[4], job[3]        # (the stepped block the constraint backward staged)
            call("nlbac_mlp_bwd_data_head", P.n_act, P.io_act, NP, B, C.byref(H), s)
        else:
            D = Do + A
            call("nlbac_gauss_sample_bwd", ws.heads2.data_ptr(), 2 * A, ws.eps[1:1 + NP].data_ptr(),
                 self.policy.action_scale.data_ptr(), A, NP * B, B, ws.dxq[0].data_ptr() + 4 * Do, D, ws.dxq[1].data_ptr() + 4 * Do,
                 D, du2.data_ptr(), du_ld, sc + 4 * SC.SC_ALPHA, 1.0 / G, ws.dheads2.data_ptr(), 2 * A, s)
            call("nlbac_mlp_bwd_data", P.n_act, P.io_act, NP, B, s)
        tune = self.automatic_entropy_tuning
        p_part_q, n_part = ws.p_part_q, ws.n_part_q
        for g, cnt, nets, gio, sk_ws in P.act_groups:
            a = g.arena
            bwd_weights(nets, gio, cnt, B, a.n_slabs, a.n, self.device, ws=sk_ws)
            la = a.theta.data_ptr() + 4 * g.la_off

            def alpha_grads(p_grad, g=g, cnt=cnt, la=la):
                # policy_loss_1 / alpha losses from the (global) partial sums; d log_alpha goes straight into
                # the gradient the Adam step reads (it is already a global mean: it must not be all-reduced).
                # Single GPU: nlbac_actor_q_terms has done this in its own launch.
                if self.world > 1:
                    call("nlbac_actor_scalars", p_part_q, n_part, G, g.first, cnt, self.target_entropy, la, g.la_stride,
                         p_grad + 4 * g.la_off, sc, s)
                if not tune:
                    z = torch.zeros(1, device=self.device)
                    for off in [g.la_off + k * g.la_stride for k in range(cnt)]:
                        call("nlbac_axpby", 0.0, z.data_ptr(), 0.0, None, 1, p_grad + 4 * off, s)
            # (alpha = exp(log_alpha) is refreshed by the thread of the Adam step that moves log_alpha)
            refresh = ([g.la_off + k * g.la_stride for k in range(cnt)],
                       [sc + 4 * (SC.SC_ALPHA + g.first + k) for k in range(cnt)]) if tune else None
            last = g is P.act_groups[-1][0]
            mir = self._readback.mirror if last else None
            self._adam(a, self.lr, a.n_slabs, before_step=alpha_grads, alpha=refresh, mirror=mir[1] if mir else None)
            if mir:
                self._readback.mirrored(mir[0])
        self._prefetch_next(ws, ws.updates_now)

    # ------------------------------------------------------------ checkpoints
    def save_model(self, output):
        print('Saving models in {}'.format(output))
        torch.save(self.policy.state_dict(), '{}/actor.pkl'.format(output))
        torch.save(self.critic.state_dict(), '{}/critic.pkl'.format(output))
        torch.save(self.lyapunovNet.state_dict(), '{}/lyapunov.pkl'.format(output))
        if self.BarrierNet is not None:
            torch.save(self.BarrierNet.state_dict(), '{}/barrier.pkl'.format(output))
        torch.save(self.neural_ode_model.state_dict(), '{}/node_model.pkl'.format(output))

    def load_weights(self, output):
        if output is None:
            return
        print('Loading models from {}'.format(output))
        dev = torch.device(self.device)
        self.policy.load_state_dict(torch.load('{}/actor.pkl'.format(output), map_location=dev, weights_only=True))
        self.critic.load_state_dict(torch.load('{}/critic.pkl'.format(output), map_location=dev, weights_only=True))
        self.lyapunovNet.load_state_dict(torch.load('{}/lyapunov.pkl'.format(output), map_location=dev, weights_only=True))
        if self.BarrierNet is not None:
            self.BarrierNet.load_state_dict(torch.load('{}/barrier.pkl'.format(output), map_location=dev, weights_only=True))
        self.repack_all()

    def load_model(self, actor_path, critic_path, lyapunov_path, barrier_path=None):
        if actor_path is not None:
            self.policy.load_state_dict(torch.load(actor_path, weights_only=True))
        if critic_path is not None:
            self.critic.load_state_dict(torch.load(critic_path, weights_only=True))
        if lyapunov_path is not None:
            self.lyapunovNet.load_state_dict(torch.load(lyapunov_path, weights_only=True))
        if barrier_path is not None and self.BarrierNet is not None:
            self.BarrierNet.load_state_dict(torch.load(barrier_path, weights_only=True))
        self.repack_all()


    # Full training state (row f4: what the reference's save_model omits — targets, optimiser moments and step counts,
    # multipliers, augmented terms, temperatures, the NODE): resume continues bit for bit.
    def save_checkpoint(self, path):
        names = ("ar_c", "ar_a", "ar_b", "ar_n")
        state = {"solver": self.solver, "sc": self.sc.cpu()}
        for n in names:
            a = getattr(self, n, None)
            if a is not None:
                state[n] = {k: getattr(a, k).cpu() for k in ("theta", "m", "v", "state")}
                if a.target is not None:
                    state[n]["target"] = a.target.cpu()
        torch.save(state, path)

    def load_checkpoint(self, path):
        state = torch.load(path, map_location="cpu", weights_only=True)
        for n, a_state in state.items():
            if n in ("solver", "sc"):
                continue
            a = getattr(self, n)
            for k, v in a_state.items():
                getattr(a, k).copy_(v)
        self.sc.copy_(state["sc"])
        self.solver = state["solver"]
        self.repack_all()


class _TargetView:
    """state_dict-style access to a target network stored in ``arena.target``."""

    def __init__(self, module, arena):
        self.module, self.arena = module, arena

    def state_dict(self):
        out = {}
        for k, p in self.module.named_parameters():
            off = self.arena.offset_of[id(p)]
            out[k] = self.arena.target[off:off + p.numel()].view(p.shape)
        return out

    def load_state_dict(self, sd):
        cur = self.state_dict()
        with torch.no_grad():
            for k, v in sd.items():
                cur[k].copy_(v)
