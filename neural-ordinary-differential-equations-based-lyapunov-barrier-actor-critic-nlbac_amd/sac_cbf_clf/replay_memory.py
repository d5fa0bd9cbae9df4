"""Replay buffer with the reference API (``push`` / ``sample`` / ``len`` /
``position``; ``U/sac_cbf_clf/replay_memory.py``) stored as preallocated
float64 numpy columns (struct of arrays) instead of a Python list of tuples:
``sample`` is one fancy-index gather per field rather than ``np.stack`` over
``batch_size`` tuples.  Index draws use ``random.sample`` like the reference,
so the same seed selects the same transitions.
"""
import random

import numpy as np

_FIELDS = ("state", "action", "reward", "constraint", "center_pos", "next_center_pos",
           "next_state", "mask", "t", "next_t")


class ReplayMemory:

    def __init__(self, capacity, seed, initial_rows=65536):
        random.seed(seed)
        self.capacity = int(capacity)
        self._rows = min(self.capacity, int(initial_rows))
        self._cols = None
        self._len = 0
        self.position = 0

    def _alloc(self, values):
        self._cols = []
        for v in values:
            a = np.asarray(0.0 if v is None else v, dtype=np.float64)
            self._cols.append(np.zeros((self._rows,) + a.shape, dtype=np.float64))

    def _grow(self):
        new_rows = min(self.capacity, self._rows * 2)
        self._cols = [np.concatenate([c, np.zeros((new_rows - self._rows,) + c.shape[1:])]) for c in self._cols]
        self._rows = new_rows

    def push(self, state, action, reward, constraint, center_pos, next_center_pos, next_state, mask,
             t=None, next_t=None):
        self._push((state, action, reward, constraint, center_pos, next_center_pos, next_state, mask, t, next_t))

    def _push(self, values):
        if self._cols is None:
            self._alloc(values)
        if self.position >= self._rows:
            self._grow()
        for c, v in zip(self._cols, values):
            c[self.position] = 0.0 if v is None else v
        self._len = max(self._len, self.position + 1)
        self.position = (self.position + 1) % self.capacity

    def sample(self, batch_size):
        idx = np.asarray(random.sample(range(self._len), batch_size), dtype=np.int64)
        return tuple(c[idx] for c in self._cols)

    def sample_windows(self, batch_size, horizon, stride=1):
        """``batch_size`` windows of ``horizon`` consecutive transitions (``stride`` rows apart): ``(fields, valid)`` —
        the field arrays of ``sample`` with a leading (H, B, ...) and valid (B,) bool.  Start rows are drawn like
        ``sample``'s; the validity rule and the rows of an invalid window are ``window_rows``'s (the device replay's
        ``nlbac_gather_windows`` applies the same rule to its float32 rows)."""
        check_windows(batch_size, horizon, stride, self._len, host_draw=True)
        idx = np.asarray(random.sample(range(self._len), batch_size), dtype=np.int64)
        nstate = len(self._cols) - 4          # (..., next_state, mask, t, next_t)
        rows, valid = window_rows(idx, horizon, stride, self._len, self.capacity, self.position,
                                  self._cols[0], self._cols[nstate])
        return tuple(c[rows] for c in self._cols), valid

    def windows_at(self, idx, horizon, stride=1):
        """``sample_windows``'s ``(fields, valid)`` for the caller's start rows ``idx`` (int64, in [0, len)): nothing is
        drawn, no generator moves (``SAC_CBF_CLF.validate_node``)."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        check_windows(max(1, len(idx)), horizon, stride, self._len, host_draw=False)
        nstate = len(self._cols) - 4
        rows, valid = window_rows(idx, horizon, stride, self._len, self.capacity, self.position,
                                  self._cols[0], self._cols[nstate])
        return tuple(c[rows] for c in self._cols), valid

    def __len__(self):
        return self._len


def check_windows(batch_size, horizon, stride, length, host_draw):
    """The argument checks of ``sample_windows`` (host and device replay), before anything touches a device."""
    for name, v in (("batch_size", batch_size), ("horizon", horizon), ("stride", stride)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("sample_windows: %s must be an integer >= 1; got %r" % (name, v))
    if host_draw and batch_size > length:
        raise ValueError("sample_windows: %d start rows drawn without replacement from %d rows" % (batch_size, length))
    if (horizon - 1) * stride >= length:
        raise ValueError("sample_windows: a window of %d steps %d rows apart spans more than the %d rows held"
                         % (horizon, stride, length))


def window_rows(idx, horizon, stride, length, capacity, position, obs, next_obs):
    """Ring rows (H, B) of the windows that start at rows ``idx`` and which of them are valid (B,).

    ``oldest = position if length == capacity else 0``; ``a0 = (idx - oldest) mod capacity`` is the start row's rank in
    push order, step k the row of rank ``a0 + k stride``.  Valid: (a) ``a0 + (H-1) stride < length`` — the window neither
    runs past the newest row nor steps over the write head — and (b) every step's ``next_obs`` is, bit for bit, the next
    step's ``obs``: a reset or a termination breaks that chain (``mask`` stays 1 at a time-limit reset and cannot tell).
    An invalid window still gets rows: step k is the row of rank ``min(a0 + k stride, length - 1)``."""
    idx = np.asarray(idx, dtype=np.int64)
    oldest = position if length == capacity else 0
    a0 = (idx - oldest) % capacity
    ranks = a0[None, :] + stride * np.arange(horizon, dtype=np.int64)[:, None]
    valid = ranks[-1] < length
    rows = (oldest + np.minimum(ranks, length - 1)) % capacity
    bits = lambda a: np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32).reshape(len(a), -1)
    for k in range(horizon - 1):
        valid &= (bits(next_obs[rows[k]]) == bits(obs[rows[k + 1]])).all(axis=1)
    return rows, valid



class DeviceReplayMemory:
    """Replay buffer resident in HBM in the agent's minibatch row layout.

    Same ``push`` / ``sample`` / ``len`` / ``position`` API as ``ReplayMemory``; rows are staged in a pinned host
    block and uploaded in chunks, and ``sample_rows`` gathers a minibatch on the device straight into the agent's
    workspace (one ``nlbac_gather_rows`` launch) — ``SAC_CBF_CLF.update_parameters`` takes that path, so an update
    moves ``8 * batch`` index bytes over PCIe instead of the whole minibatch.  Index draws use ``random.sample`` on
    the host exactly like the reference (``replay_memory.py:22``), so the same seed selects the same transitions;
    ``device_rng=True`` draws them on the device instead (with replacement, no host involvement): index draw, gather
    and — when the caller hands in the agent's noise buffer (``eps_out``) — the update's N(0,1) policy noise are one
    ``nlbac_sample_rows`` launch.
    """

    def __init__(self, capacity, seed, agent, chunk=4096, device_rng=False):
        import torch
        random.seed(seed)
        self.capacity, self.agent, self.device_rng = int(capacity), agent, device_rng
        self.lay, self.device = agent.lay, agent.device
        self.n_fields = 11 if self.lay.sig is not None else 10
        self.rows = torch.zeros(self.capacity, self.lay.LD, dtype=torch.float32, device=self.device)
        self._stage = torch.zeros(min(chunk, self.capacity), self.lay.LD, dtype=torch.float32).pin_memory() \
            if torch.cuda.is_available() else torch.zeros(min(chunk, self.capacity), self.lay.LD)
        self._stage_np = self._stage.numpy()
        self._n_staged, self._stage_start = 0, 0
        self._len = 0
        self.position = 0
        self._seed = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF   # Philox key
        self._draws = 0                                                                           # Philox counter

    def push(self, *fields, t=None, next_t=None):
        """Positional fields in the order of the reference's ``push`` (10, or 11 with the barrier signal)."""
        fields = tuple(fields)
        if len(fields) == self.n_fields - 2:
            fields = fields + (t, next_t)
        assert len(fields) == self.n_fields, "push takes %d fields" % self.n_fields
        if self._n_staged == self._stage_np.shape[0] or \
                (self._n_staged and self._stage_start + self._n_staged != self.position):
            self.flush()
        if self._n_staged == 0:
            self._stage_start = self.position
        batch1 = tuple(np.asarray(0.0 if f is None else f, dtype=np.float64)[None] for f in fields)
        self._stage_np[self._n_staged] = self.agent._rows_from_host(batch1).numpy()[0]
        self._n_staged += 1
        self._len = max(self._len, self.position + 1)
        self.position = (self.position + 1) % self.capacity
        if self.position == 0:
            self.flush()                       # keep a staged run contiguous in the ring

    def push_rows(self, rows):
        """Bulk insert of minibatch-layout rows (host or device tensor, (n, LD))."""
        import torch
        rows = torch.as_tensor(rows, dtype=torch.float32)
        n = rows.shape[0]
        assert rows.shape[1] == self.lay.LD and n <= self.capacity
        if n == 0:
            self.flush()
            return
        start = self.reserve_rows(n)
        first = min(n, self.capacity - start)
        self.rows[start:start + first].copy_(rows[:first])
        if n > first:
            self.rows[:n - first].copy_(rows[first:])

    def reserve_rows(self, n):
        """The bookkeeping of ``push_rows`` for ``n`` rows a kernel writes in place: returns the first ring row (row k of
        the push is ring row ``(first + k) mod capacity``)."""
        self.flush()
        n = int(n)
        assert 0 < n <= self.capacity
        first = self.position
        self._len = min(self.capacity, max(self._len, self.position + n))
        self.position = (self.position + n) % self.capacity
        return first

    def flush(self):
        if self._n_staged:
            self.rows[self._stage_start:self._stage_start + self._n_staged].copy_(self._stage[:self._n_staged],
                                                                                 non_blocking=False)
            self._n_staged = 0

    def sample_rows(self, batch_size, out=None, eps_out=None):
        """Minibatch-layout rows (batch_size, LD) on the device.  ``eps_out``: a contiguous fp32 device buffer to fill
        with N(0,1) draws alongside (``SAC_CBF_CLF.update_on_device(..., eps_ready=True)`` then skips its own draw)."""
        import torch
        from .. import _lib
        from ..arena import stream_ptr
        self.flush()
        if out is None:
            out = torch.empty(batch_size, self.lay.LD, dtype=torch.float32, device=self.device)
        if self.device_rng:
            self._draws += 1
            _lib.call("nlbac_sample_rows", self.rows.data_ptr(), self._len, self.lay.LD, batch_size, out.data_ptr(),
                      eps_out.data_ptr() if eps_out is not None else None,
                      eps_out.numel() if eps_out is not None else 0, self._seed, self._draws, stream_ptr())
            return out
        idx = torch.tensor(random.sample(range(self._len), batch_size), dtype=torch.int64).to(self.device)
        _lib.call("nlbac_gather_rows", self.rows.data_ptr(), self._len, self.lay.LD, idx.data_ptr(), batch_size,
                  out.data_ptr(), stream_ptr())
        if eps_out is not None:
            eps_out.normal_()
        return out

    def sample_windows(self, batch_size, horizon, stride=1, out=None, idx=None):
        """``batch_size`` trajectory windows of ``horizon`` consecutive rows (``stride`` rows apart: 1, or the lane count
        of a driver that pushes one row per lane per step): ``(rows (H, B, LD), valid (B,) float 1 / 0)`` on the device,
        one ``nlbac_gather_windows`` launch (its header comment has the validity rule; ``window_rows`` above is the same
        rule in numpy).  Start rows: ``random.sample`` on the host like ``sample_rows``; with ``device_rng`` drawn by the
        launch itself (``nlbac_sample_windows``, with replacement); ``idx`` (int64 tensor, host or device): the caller's.
        The launch's per-block counts of valid windows stay in ``self.window_counts`` for the loss that follows."""
        import torch
        from .. import _lib
        from ..arena import stream_ptr
        check_windows(batch_size, horizon, stride, self._len, host_draw=idx is None and not self.device_rng)
        if idx is not None:
            idx = torch.as_tensor(idx)
            if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() != batch_size:
                raise ValueError("sample_windows: idx must be %d int64 start rows" % batch_size)
        if out is not None and (tuple(out.shape) != (horizon, batch_size, self.lay.LD) or not out.is_contiguous()
                                or out.dtype != torch.float32):
            raise ValueError("sample_windows: out must be a contiguous float32 (%d, %d, %d) tensor"
                             % (horizon, batch_size, self.lay.LD))
        self.flush()
        lay = self.lay
        if out is None:
            out = torch.empty(horizon, batch_size, lay.LD, dtype=torch.float32, device=self.device)
        valid = torch.empty(batch_size, dtype=torch.float32, device=self.device)
        self.window_counts = counts = torch.empty((batch_size + 255) // 256, dtype=torch.int32, device=self.device)
        ring = (self.rows.data_ptr(), self._len, self.capacity, self.position, lay.LD)
        tail = (horizon, stride, lay.obs, lay.nobs, lay.obs_dim, out.data_ptr(), valid.data_ptr(), counts.data_ptr())
        if idx is None and self.device_rng:
            self._draws += 1
            _lib.call("nlbac_sample_windows", *ring, batch_size, *tail, self._seed, self._draws, stream_ptr())
            return out, valid
        if idx is None:
            idx = torch.tensor(random.sample(range(self._len), batch_size), dtype=torch.int64)
        idx = idx.to(self.device)
        _lib.call("nlbac_gather_windows", *ring, idx.data_ptr(), batch_size, *tail, stream_ptr())
        return out, valid

    def sample(self, batch_size):
        """Reference-shaped ``sample``: the 10 (11) stacked numpy arrays (device -> host; use ``sample_rows`` on the
        update path)."""
        rows = self.sample_rows(batch_size).cpu().numpy().astype(np.float64)
        lay = self.lay
        cols = [("obs", lay.obs_dim), ("act", lay.act_dim), ("rew", 0), ("con", 0)]
        if lay.sig is not None:
            cols.append(("sig", 0))
        cols += [("lya", lay.lya_dim), ("nlya", lay.lya_dim), ("nobs", lay.obs_dim), ("mask", 0), ("t", 0), ("nt", 0)]
        out = []
        for name, w in cols:
            c = getattr(lay, name)
            out.append(rows[:, c] if w == 0 else rows[:, c:c + w])
        return tuple(out)

    def __len__(self):
        return self._len


class DeviceKeptReplay:
    """The controller replay of the vectorised driver with hand-over (``vector_handover.VectorHandover.push``): a ring in
    HBM that receives, per vector step, the rows of the lanes in which the primary controller acted — how many is decided
    on the device, so the ring's head ``{position, length}`` lives in device memory (``head``, (2, 2) int64: two copies,
    ``half`` names the current one; an append reads it and writes the other, the host only alternates ``half``).

    ``sample_rows`` draws on the device through ``nlbac_sample_rows_head``, which reads the length from the head: no
    index and no length passes through the host.  ``draws_from`` is the NODE replay of the same run: the two share its
    Philox key and its one draw counter, so a run whose hand-over never fires draws exactly what a single
    ``DeviceReplayMemory`` serving both purposes draws.  ``len()`` is a cached lower bound (the length never shrinks);
    ``refresh_len()`` reads the head and is the only host read."""
    device_rng = True

    def __init__(self, capacity, seed, agent, draws_from):
        import torch
        self.capacity, self.agent, self.draws_from = int(capacity), agent, draws_from
        self.seed = seed           # (kept for the record: the Philox key is draws_from's)
        self.lay, self.device = agent.lay, agent.device
        self.rows = torch.zeros(self.capacity, self.lay.LD, dtype=torch.float32, device=self.device)
        self.head = torch.zeros(2, 2, dtype=torch.int64, device=self.device)
        self.half = 0
        self._len = 0

    def refresh_len(self):
        """Read the current head's length (a host sync); ``len()`` answers with it from then on."""
        self._len = max(self._len, int(self.head[self.half, 1]))
        return self._len

    def sample_rows(self, batch_size, out=None, eps_out=None):
        """``DeviceReplayMemory.sample_rows`` in its ``device_rng`` mode, on the length the device holds."""
        import torch
        from .. import _lib
        from ..arena import stream_ptr
        if out is None:
            out = torch.zeros(batch_size, self.lay.LD, dtype=torch.float32, device=self.device)
        src = self.draws_from
        src._draws += 1
        _lib.call("nlbac_sample_rows_head", self.rows.data_ptr(), self.head.data_ptr(), self.half, self.capacity,
                  self.lay.LD, batch_size, out.data_ptr(), eps_out.data_ptr() if eps_out is not None else None,
                  eps_out.numel() if eps_out is not None else 0, src._seed, src._draws, stream_ptr())
        return out

    def sample(self, batch_size):
        raise NotImplementedError("DeviceKeptReplay.sample: the length of this replay is known on the device only, so "
                                  "there is no host index draw and no host copy of a minibatch; use sample_rows")

    def __len__(self):
        return self._len
