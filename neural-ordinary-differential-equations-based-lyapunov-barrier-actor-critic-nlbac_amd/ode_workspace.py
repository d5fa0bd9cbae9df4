"""Device memory of the NODE solvers (``odeint.py``): the step slots of an RK step carved out of per-capacity pools,
and the named scratch buffers of a solve size.  ``SolverWorkspaces`` is the allocator half of a solver."""
import ctypes as C

import torch

from . import _lib


class _Carver:
    """Hands out the buffers of ONE step slot: consecutive 16-byte-aligned pieces of a flat float32 slice.  Every slot
    of a pool is carved by the same sequence of requests, so a buffer sits at the same offset in every slot — which is
    what lets the device-driven dopri5 chain address "the same buffer, k slots further" by pointer arithmetic
    (``nlbac_rk_chain.slot_floats``).  ``flat is None``: dry run, only counts."""

    def __init__(self, flat, device):
        self.flat, self.device, self.k = flat, device, 0

    def zeros(self, *shape, dtype=torch.float32):
        numel = 1
        for d in shape:
            numel *= d
        take = (numel + 3) & ~3
        off, self.k = self.k, self.k + take
        if self.flat is None:
            return torch.empty(0, dtype=dtype)
        assert self.k <= self.flat.numel(), "step slot too small"
        t = self.flat[off:off + numel]
        if dtype != torch.float32:
            t = t.view(dtype)
        return t.view(*shape)


class _SlotPool:
    """Step slots of one capacity bucket: chunks of ``slots_per_chunk`` slots, each chunk ONE allocation
    [slots][slot_floats].  The device-driven chain works inside chunk 0 (contiguous, ``n_slots`` = its size); the
    host-driven path just asks for the next slot and may spill into further chunks."""

    def __init__(self, solver, cap, S, n_slots, dry_only=False):
        self.solver, self.cap, self.S, self.n_slots = solver, cap, S, n_slots
        dry = _Carver(None, solver.device)
        solver.STEP_WS(solver, cap, S, dry).bwd(solver)
        self.slot_floats = (dry.k + 63) & ~63
        if dry_only:
            return
        self.chunks = [torch.zeros(n_slots, self.slot_floats, dtype=torch.float32, device=solver.device)]
        self.views = {}                  # (n, idx) -> step workspace

    def ws(self, n, idx):
        assert n <= self.cap
        w = self.views.get((n, idx))
        if w is None:
            c, i = divmod(idx, self.n_slots)
            while c >= len(self.chunks):
                self.chunks.append(torch.zeros(self.n_slots, self.slot_floats, dtype=torch.float32,
                                               device=self.solver.device))
            for k in [k for k in self.views if k[0] != n]:      # views laid out for another row count go
                del self.views[k]
            w = self.views[(n, idx)] = self.solver.STEP_WS(self.solver, n, self.S, _Carver(self.chunks[c][i], self.solver.device))
            w.slot, w.pool = idx, self
        return w


class _StepWS:
    """Device buffers of one RK step for n rows (stage-major)."""
    # what a per-problem solver takes over from a joint first attempt: (buffer, leading blocks per row range)
    ADOPT = ("K", "Y", "gout", "err", "acts_f", "acts_g")

    def __init__(self, solver, n, S, store):
        dev, ns, nu = solver.device, solver.n_s, solver.n_u
        f, g = solver.f, solver.g
        self.n, self.S = n, S
        self._store = store
        z = self._store.zeros
        self.K = z(S, n, ns)
        self.Y = z(S, n, ns)
        self.fout = z(n, ns)
        self.gout = z(S, n, ns * nu)
        # a rollout that is only differentiated w.r.t. its inputs keeps bit-packed ReLU masks (one uint32 per 32
        # hidden units) instead of the activations: 1/32 of the HBM traffic of the fused step kernels
        self.bits = bool(solver.fused and not solver.keep_acts)
        if self.bits:
            zi = lambda *s: self._store.zeros(*s, dtype=torch.int32)
            # words per row and layer: one per 32 hidden units, or (register-resident kernels) one per lane quarter
            lib = _lib.load()
            self.wf = lib.nlbac_node_rk_mask_words(C.byref(f.desc), C.byref(g.desc), 0)
            self.wg = lib.nlbac_node_rk_mask_words(C.byref(f.desc), C.byref(g.desc), 1)
            self.acts_f = zi(f.n_layers - 1, S * n, self.wf)
            self.acts_g = zi(g.n_layers - 1, S * n, self.wg)
        else:
            self.wf, self.wg = f.hid, g.hid
        # rows + words (acts_bits 2, the NODE fit on the register-resident kernels): the forward also leaves the ReLU
        # mask words, which the backward gates on; the weight gradients read the rows.  Each net's words
        # [layer][S*n][4] sit directly behind its rows — where nlbac_node_rk_fwd / _bwd look for them
        self.words = not self.bits and solver._fit_words_on()
        self.acts_bits = 1 if self.bits else (2 if self.words else 0)
        if not self.bits:       # (hid % 4 == 0: the rows fill their carve, the words start where they end)
            mw = lambda net: self._store.zeros(net.n_layers - 1, S * n, 4, dtype=torch.int32) if self.words else None
            self.acts_f = z(f.n_layers - 1, S * n, f.hid)
            self.mw_f = mw(f)
            self.acts_g = z(g.n_layers - 1, S * n, g.hid)
            self.mw_g = mw(g)
        if self.words:
            self.ADOPT = _StepWS.ADOPT + ("mw_f", "mw_g")
        self.y1 = z(n, ns)
        self.err = z(n, ns)
        self._bwd = None
        self.io_fwd, self.io_bwd = {}, {}

    def bwd(self, solver):
        if self._bwd is None:
            dev, ns, nu, n, S = solver.device, solver.n_s, solver.n_u, self.n, self.S
            f, g = solver.f, solver.g
            z = self._store.zeros
            self.dK = z(S, n, ns)
            keep = solver.keep_acts or not solver.fused      # weight gradients / the stage-by-stage path need dz
            self.dG = z(S, n, ns * nu) if keep else None
            self.dz_f = z(f.n_layers - 1, S * n, f.hid) if keep else None
            self.dz_g = z(g.n_layers - 1, S * n, g.hid) if keep else None
            self.dXf = z(n, f.in_dim)
            self.dXg = z(n, g.in_dim)
            self.dy0 = z(n, ns)
            self.dy1 = z(n, ns)
            self._bwd = True
        return self


class _ConcatStepWS:
    """The same for the single-net field ``dx/dt = net([x, c])`` (``ConcatNodeSolver``)."""
    ADOPT = ("K", "Y", "err", "acts")

    def __init__(self, solver, n, S, store):
        dev, ns, nc = solver.device, solver.n_s, solver.n_u
        net = solver.net
        self.n, self.S = n, S
        self._store = store
        z = self._store.zeros
        self.K = z(S, n, ns)
        self.Y = z(S, n, ns)
        # a rollout that is only differentiated w.r.t. its inputs keeps ReLU mask words instead of the activations, where
        # the fused kernels can (the register-resident ones: nlbac_concat_rk_mask_words)
        words = _lib.load().nlbac_concat_rk_mask_words(C.byref(net.desc)) if (solver.fused and not solver.keep_acts) else 0
        self.bits = words > 0
        if self.bits:
            self.wa = words
            self.acts = self._store.zeros(net.n_layers - 1, S * n, words, dtype=torch.int32)
        else:
            self.wa = net.hid
            self.acts = z(net.n_layers - 1, S * n, net.hid)
        self.y1 = z(n, ns)
        self.err = z(n, ns)
        self.io_fwd, self.io_bwd = {}, {}
        self._bwd = None
        # a normalised field keeps the normalised net inputs of every stage for the first layer's weight gradient
        self.Xn = z(S, n, net.in_dim) if solver.norm is not None else None

    def bwd(self, solver):
        if self._bwd is None:
            dev, ns, nc, n, S = solver.device, solver.n_s, solver.n_u, self.n, self.S
            net = solver.net
            z = self._store.zeros
            self.dK = z(S, n, ns)
            self.dz = z(net.n_layers - 1, S * n, net.hid)
            self.dX = z(n, net.in_dim)
            self.dy0 = z(n, ns)
            self.dy1 = z(n, ns)
            self.c_rep = z(S * n, nc)      # carried inputs repeated per stage (first-layer weight gradients)
            self.dyn = z(S, n, ns) if solver.norm is not None else None      # d/d(net output) = dK * out_std
            self._bwd = True
        return self


class SolverWorkspaces:
    """Allocator of a solver (a base class of ``AffineNodeSolver``): slot pools by capacity bucket, scratch by row count.
    The solver supplies ``device``, ``n_s``, ``fused``, ``keep_acts``, ``STEP_WS`` and ``_fit_words_on()``."""

    def _init_workspaces(self):
        self._ws = {}          # (n, S, idx) -> _StepWS
        self._scratch = {}     # row count -> {(name, shape, dtype) -> buffer}
        self._pools = {}       # (bucket, S, fused, keep_acts, words) -> _SlotPool
        self._n_order = []     # row counts, least recently used first
        self._cur_n = 0        # row count of the current solve
        self.generation = 0    # bumped whenever device buffers are freed or re-laid-out (owners of hipGraphs watch it)
        self.out_into = None   # the owner's tensor for the next solves' result (see ``_out_buf``)

    MAX_SIZES = 2      # distinct row counts whose buffers are kept (the NODE fit's batch grows with the replay)

    def _touch(self, n):
        """Start of a solve on n rows: make n the current size and drop the scratch of the least recently used sizes
        beyond ``MAX_SIZES`` — a training run feeds the NODE fit min(replay size, 32768) rows, a new count at every fit
        while the replay fills.  (Step slots live in per-capacity pools, see ``_pool``.)"""
        order = self._n_order
        if n in order:
            order.remove(n)
        order.append(n)
        while len(order) > self.MAX_SIZES:
            old = order.pop(0)
            self._scratch.pop(old, None)
            self.generation += 1
        self._cur_n = n

    @staticmethod
    def _bucket(n):
        return n if n <= 4096 else -(-n // 4096) * 4096

    DEFAULT_SLOTS = 4      # step slots of a pool's first chunk = steps the device-driven chain can accept without a restart

    def _pool(self, n, S, min_slots=1):
        """The slot pool serving n rows / S stages (one per capacity bucket and solver mode; the two most recently
        used buckets are kept).  ``generation`` counts every event that frees or re-lays-out device buffers — captured
        hipGraphs bake their addresses in and are dropped by their owners when it moves."""
        pools = self._pools
        key = (self._bucket(n), S, self.fused, self.keep_acts, self._fit_words_on())
        pool = pools.get(key)
        dropped = False
        if pool is not None and pool.n_slots < min_slots:
            del pools[key]
            pool, dropped = None, True
        if pool is None:
            buckets = list(dict.fromkeys(k[0] for k in pools))              # in order of first use
            if key[0] not in buckets and len(buckets) >= self.MAX_SIZES:
                for k in [k for k in pools if k[0] == buckets[0]]:         # the oldest bucket goes, whole
                    del pools[k]
                dropped = True
            if dropped:
                self.generation += 1
                # pools are GB-sized and each regrowth asks for a new size: hand the freed blocks back to the driver,
                # or the caching allocator keeps every size it has ever seen (279 GiB reserved for 39 GiB in use in a
                # long dopri5 training run before this)
                if not torch.cuda.is_current_stream_capturing():
                    torch.cuda.empty_cache()
            n_slots = max(min_slots, self.DEFAULT_SLOTS if S == 7 else 1)
            pool = _SlotPool(self, key[0], S, n_slots, dry_only=True)
            if pool.slot_floats * 4 * n_slots > self.MAX_POOL_BYTES:
                raise _lib.NlbacError(
                    "dopri5: %d accepted steps of %d rows need %.0f GiB of step slots (limit %.0f GiB): the field has "
                    "become stiff for back-propagation through the steps — use the adjoint (agent.adjoint = True / "
                    "odeint_adjoint), whose memory does not grow with the step count"
                    % (n_slots, key[0], pool.slot_floats * 4 * n_slots / 2 ** 30, self.MAX_POOL_BYTES / 2 ** 30))
            pool = pools[key] = _SlotPool(self, key[0], S, n_slots)
        return pool

    MAX_POOL_BYTES = 128 * 2 ** 30

    def _step_ws(self, n, S, idx):
        pool = self._pool(n, S)
        had = (n, idx) in pool.views
        ws = pool.ws(n, idx)
        if not had and any(k[0] != n for k in pool.views):
            self.generation += 1
        return ws

    def _out_buf(self, n, fallback=None):
        """Where the solve's result goes: the caller's tensor (``out_into``, when it has the solve's shape — the next
        launches read it there, no copy) or a solver-owned buffer."""
        t = self.out_into
        if t is not None and tuple(t.shape) == (n, self.n_s) and t.is_contiguous():
            return t
        return fallback if fallback is not None else self._buf("dopri_out", n, self.n_s)

    def _buf(self, name, *shape, dtype=torch.float32):
        """Named scratch buffer of the current solve size (dropped with that size's workspaces, see ``_touch``)."""
        pool = self._scratch.setdefault(self._cur_n, {})
        key = (name, shape, dtype)
        if key not in pool:
            pool[key] = torch.zeros(*shape, dtype=dtype, device=self.device)
        return pool[key]
