"""Backup-controller hand-over of the vectorised driver (``train.train_vectorized(handover=...)``) on the device.

Lane ``i`` is ``train.train``'s loop for one environment as far as controllers and replays go: ``flags[i]`` is
``make_handover(env_name, env, True).use_backup`` as ``train`` evaluates it before the action of a step, with
``begin_episode(e)`` called with the lane's own count of finished episodes.  One launch per vector step
(``nlbac_vector_step_rows``) runs ``on_backup_action`` / ``after_step`` / ``begin_episode`` for every lane, assembles the
transition rows in the NODE replay's ring and marks the rows the primary controller produced; a second one
(``nlbac_ring_append_kept``) compacts those, in lane order, into the controller replay, whose head lives in device
memory.  Nothing of a transition or of a decision reaches the host.  The thresholds and caps are the host classes'
attributes (``params_for``): the constants live in ``train.py`` alone.
"""
import ctypes as C

from . import _lib

KINDS = {"Unicycle": 0, "SimulatedCars": 1, "Pvtol": 2}


def params_for(env_name, env=None, **overrides):
    """``_lib.HandoverParams`` for ``env_name`` from the attributes of its host class (``train._UnicycleHandover`` /
    ``_CarsHandover`` / ``_PvtolHandover``) and ``env.operator_dist`` (Pvtol); ``overrides``: fields to set otherwise
    (tests: ``first_backup_episode=2**30`` never hands over)."""
    from . import train
    if env_name not in KINDS:
        raise ValueError("no backup-controller hand-over for %r (the copies with one: %s)" % (env_name, ", ".join(KINDS)))
    cls = {"Unicycle": train._UnicycleHandover, "SimulatedCars": train._CarsHandover, "Pvtol": train._PvtolHandover}[env_name]
    p = _lib.HandoverParams()
    p.kind = KINDS[env_name]
    p.first_backup_episode, p.memory_t_shift = cls.first_backup_episode, cls.memory_t_shift
    p.min_check_step, p.lookback = cls.MIN_CHECK_STEP, cls.LOOKBACK
    if env_name == "Unicycle":
        p.stuck2, p.checks, p.max_backup, p.away2 = cls.STUCK2, cls.CHECKS, cls.MAX_BACKUP, cls.AWAY2
    elif env_name == "SimulatedCars":
        p.gap, p.max_backup, p.min_backup = cls.GAP, cls.MAX_BACKUP, cls.MIN_BACKUP
    else:
        p.stuck2, p.checks, p.max_backup, p.away2 = cls.STUCK2, cls.CHECKS, cls.MAX_BACKUP, cls.AWAY2
        p.run_checks, p.run_max_backup, p.back_frac, p.x_mid = cls.RUN_CHECKS, cls.RUN_MAX_BACKUP, cls.BACK_FRAC, cls.X_MID
        if env is None or not hasattr(env, "operator_dist"):
            raise ValueError("params_for('Pvtol', env): the environment's operator_dist is one of the thresholds")
        p.operator_dist = float(env.operator_dist)
    names = {f[0] for f in _lib.HandoverParams._fields_}
    for k, v in overrides.items():
        if k not in names or k == "kind":
            raise ValueError("params_for: no such field %r" % k)
        setattr(p, k, min(int(v), 2 ** 31 - 1) if isinstance(getattr(p, k), int) else float(v))
    return p


def row_layout(lay):
    """``_lib.RowLayout`` of a minibatch layout (``update_plan._Layout``)."""
    r = _lib.RowLayout()
    r.obs_dim, r.act_dim, r.lya_dim, r.ld = lay.obs_dim, lay.act_dim, lay.lya_dim, lay.LD
    for k in ("obs", "act", "rew", "con", "lya", "nlya", "nobs", "mask", "t", "nt"):
        setattr(r, k, getattr(lay, k))
    return r


class VectorHandover:
    """The lane state of ``n`` hand-over state machines and ``flags`` ((n,) bool on the device: the backup controller
    acts in that lane at the next step).  ``step``: the state machine alone; ``push``: the fused path of the driver."""

    def __init__(self, env_name, n, device, params=None):
        import torch
        if env_name not in KINDS:
            raise ValueError("no backup-controller hand-over for %r (the copies with one: %s)" % (env_name, ", ".join(KINDS)))
        self.params = params if params is not None else params_for(env_name)
        if self.params.kind != KINDS[env_name]:
            raise ValueError("hand-over parameters of kind %d for %s" % (self.params.kind, env_name))
        if not (1 <= self.params.lookback <= _lib.HANDOVER_RING and self.params.min_check_step >= self.params.lookback):
            raise ValueError("hand-over parameters: 1 <= lookback <= %d and min_check_step >= lookback" % _lib.HANDOVER_RING)
        self.n, self.device = int(n), torch.device(device)
        if not 1 <= self.n <= 65536:
            raise ValueError("VectorHandover: 1 <= n <= 65536 lanes")
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=self.device)
        self.pos_ring = z(_lib.HANDOVER_RING, 2, self.n, dtype=torch.float64) if self.params.kind != 1 else None
        self.istate = z(_lib.HANDOVER_ISTATE, self.n, dtype=torch.int32)
        self.dstate = z(2, self.n, dtype=torch.float64)
        self.istate[7] = int(self.params.first_backup_episode <= 0)      # begin_episode(0)
        self.flags = z(self.n, dtype=torch.bool)
        self.kept = z(self.n, dtype=torch.uint8)
        self.counts = z((self.n + 255) // 256, dtype=torch.int32)
        self._layouts = {}

    def _launch(self, lay, lya_pre, lya_next, obs_next, info0, done, ep_step, row_inputs, dt, max_steps, ring):
        from .arena import stream_ptr
        key = id(lay)
        if key not in self._layouts:
            self._layouts[key] = (lay, lay if isinstance(lay, _lib.RowLayout) else row_layout(lay))
        rl = self._layouts[key][1]
        for name, x, w in (("lya_pre", lya_pre, rl.lya_dim), ("lya_next", lya_next, rl.lya_dim), ("obs_next", obs_next, rl.obs_dim)):
            if tuple(x.shape) != (self.n, w) or not x.is_contiguous() or x.dtype.itemsize != 8:
                raise ValueError("VectorHandover: %s must be a contiguous float64 (%d, %d) tensor" % (name, self.n, w))
        for name, x in (("done", done), ("ep_step", ep_step)):
            if x.numel() != self.n or not x.is_contiguous() or x.dtype.itemsize != 4:
                raise ValueError("VectorHandover: %s must be a contiguous int32 (%d,) tensor" % (name, self.n))
        if info0.dim() != 1 or info0.shape[0] != self.n or info0.dtype.itemsize != 8:
            raise ValueError("VectorHandover: info0 must be a float64 (%d,) tensor (a column view is fine)" % self.n)
        reward, constraint, obs_prev, action = row_inputs
        ptr = lambda x: None if x is None else x.data_ptr()
        _lib.call("nlbac_vector_step_rows", self.n, C.byref(self.params), C.byref(rl), lya_pre.data_ptr(),
                  lya_next.data_ptr(), obs_next.data_ptr(), ptr(reward), ptr(constraint), info0.data_ptr(),
                  int(info0.stride(0)), done.data_ptr(), ep_step.data_ptr(), ptr(obs_prev), ptr(action), float(dt),
                  int(max_steps), *ring, ptr(self.pos_ring), self.istate.data_ptr(), self.dstate.data_ptr(),
                  self.flags.data_ptr(), self.kept.data_ptr(), self.counts.data_ptr(), stream_ptr())

    def step(self, lay, lya_pre, lya_next, obs_next, info0, done, ep_step):
        """The state machine alone: ``on_backup_action`` (where ``flags`` is set), ``after_step(ep_step, ...)`` and, at
        ``done``, ``begin_episode`` for every lane; ``flags`` is then the answer for the next step.  ``lay``: a layout
        (or ``_lib.RowLayout``) for the widths of the inputs."""
        self._launch(lay, lya_pre, lya_next, obs_next, info0, done, ep_step, (None,) * 4, 0.0, 0, (None, 0, 0))
        return self.flags

    def push(self, node_replay, kept_replay, obs_prev, action, reward, constraint, lya_pre, lya_next, obs_next, info0,
             done, ep_step, dt, max_steps):
        """One vector step of the driver: the transition rows go into ``node_replay``'s ring (a ``DeviceReplayMemory``,
        every lane), the rows of the lanes whose flag was clear behind ``kept_replay``'s head (a ``DeviceKeptReplay``,
        in lane order, stamps shifted by ``memory_t_shift``), the state machines advance.  Two launches.  Returns the
        first ring row of ``node_replay`` that was written."""
        from .arena import stream_ptr
        lay, n = node_replay.lay, self.n
        for name, x, w in (("obs_prev", obs_prev, lay.obs_dim), ("action", action, lay.act_dim)):
            if tuple(x.shape) != (n, w) or not x.is_contiguous() or x.dtype.itemsize != 4 or not x.dtype.is_floating_point:
                raise ValueError("VectorHandover.push: %s must be a contiguous float32 (%d, %d) tensor" % (name, n, w))
        for name, x in (("reward", reward), ("constraint", constraint)):
            if x.numel() != n or not x.is_contiguous() or x.dtype.itemsize != 8:
                raise ValueError("VectorHandover.push: %s must be a contiguous float64 (%d,) tensor" % (name, n))
        if kept_replay.lay.LD != lay.LD or n > kept_replay.capacity or n > node_replay.capacity:
            raise ValueError("VectorHandover.push: %d lanes need two rings of at least as many rows and one row layout" % n)
        first = node_replay.reserve_rows(n)
        self._launch(lay, lya_pre, lya_next, obs_next, info0, done, ep_step, (reward, constraint, obs_prev, action), dt,
                     max_steps, (node_replay.rows.data_ptr(), first, node_replay.capacity))
        half = kept_replay.half
        _lib.call("nlbac_ring_append_kept", n, self.kept.data_ptr(), self.counts.data_ptr(), node_replay.rows.data_ptr(),
                  first, node_replay.capacity, kept_replay.rows.data_ptr(), kept_replay.capacity, lay.LD,
                  kept_replay.head.data_ptr(), half, ep_step.data_ptr(), int(self.params.memory_t_shift), float(dt),
                  lay.t, lay.nt, stream_ptr())
        kept_replay.half = 1 - half
        return first

    def backup_steps(self):
        """Steps on which the backup controller acted, over all lanes (a host read)."""
        return int(self.istate[8].sum())
