"""Per-episode ledger of the vectorised driver (``train.train_vectorized(episodes=...)``, ``train.evaluate_vectorized``).

The reference's ``main.py`` logs per episode its reward, length, number of safety violations and safety cost, and
``train.train`` returns the same records.  ``EpisodeLedger`` keeps them for ``n`` lanes on the device: one launch per
vector step (``nlbac_episode_step``) adds the step's reward, ``num_safety_violation`` and ``safety_cost`` to the lane's
running episode — float64, plain adds in step order, the bits a host loop over the same numbers gets — and a second one
(``nlbac_episode_append``) writes one record per finished lane into a ring, in lane order within the vector step, behind
a head that lives in device memory.  Nothing of a transition or of a decision reaches the host; the host reads the log
when it wants it (``records``: one copy) and the sums over all lanes (``totals``: one small copy).

A record's ``goal_met`` is the simulator's ``info[:, 0]`` of the episode's last step and ``timeout`` says that the step
counter had reached the limit.  An episode that a simulator ends for another reason — the Quadrotor-like task's crash,
a true termination with mask 0 — is a record with ``goal_met = 0`` and ``timeout = 0``.
"""
import ctypes as C

import numpy as np

from . import _lib

# ``struct nlbac_episode_record`` (include/nlbac_hip.h), field for field
RECORD_DTYPE = np.dtype([("ret", "<f8"), ("safety_cost", "<f8"), ("violations", "<f8"), ("info0", "<f8"),
                         ("length", "<i4"), ("lane", "<i4"), ("lane_episode", "<i4"), ("vstep", "<i4"),
                         ("updates", "<i4"), ("timeout", "<i4"), ("backup_steps", "<i4"), ("reserved", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_lib.EpisodeRecord) == 64
_HEAD_WORDS = 8                      # int64 words in front of the ring: the (2, 2) head and padding to 64 bytes
_REC_WORDS = RECORD_DTYPE.itemsize // 8
HISTORY_KEYS = ("episode", "reward", "length", "violations", "safety_cost", "goal_met", "timeout", "lane", "lane_episode",
                "total_steps", "updates", "backup_steps")
MAX_LANES = 65536


def history_of(arrays):
    """The list-of-dicts view of ``records``' arrays, in the shape of ``train.train``'s history."""
    cast = {"reward": float, "safety_cost": float}
    cols = [(k, [cast.get(k, int)(v) for v in arrays[k]]) for k in HISTORY_KEYS]
    return [dict((k, c[j]) for k, c in cols) for j in range(len(arrays["episode"]))]


class EpisodeLedger:
    """Per-lane episode accumulators and the log of finished episodes for ``n`` lanes on ``device``.

    ``capacity``: records the ring holds (default ``max(4 n, 4096)``, at least ``n``); the log itself is unbounded —
    ``total`` counts every record ever written — and ``records(since)`` serves the last ``capacity`` of them."""

    def __init__(self, n, device, capacity=None):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_LANES:
            raise ValueError("EpisodeLedger: 1 <= n <= %d lanes (got %r)" % (MAX_LANES, n))
        n = int(n)
        if capacity is None:
            capacity = max(4 * n, 4096)
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or int(capacity) < n:
            raise ValueError("EpisodeLedger: capacity must be an int of at least n = %d records (got %r)" % (n, capacity))
        import torch
        self.n, self.capacity, self.device = n, int(capacity), torch.device(device)
        # one buffer each for what the host reads in one copy: {head, ring} and {float64 state, int32 state}
        self._log = torch.zeros(_HEAD_WORDS + self.capacity * _REC_WORDS, dtype=torch.int64, device=self.device)
        self.head = self._log[:4].view(2, 2)
        self._ring = self._log[_HEAD_WORDS:]
        words = _lib.EPISODE_DSTATE * n + (_lib.EPISODE_ISTATE * n + 1) // 2
        self._state = torch.zeros(words, dtype=torch.int64, device=self.device)
        self._dstate = self._state[:_lib.EPISODE_DSTATE * n].view(torch.float64).view(_lib.EPISODE_DSTATE, n)
        self._istate = self._state[_lib.EPISODE_DSTATE * n:].view(torch.int32)[:_lib.EPISODE_ISTATE * n].view(
            _lib.EPISODE_ISTATE, n)
        self.lane_episodes = self._istate[4]          # (n,) int32 on the device: finished episodes per lane
        self._fin = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._counts = torch.zeros((n + 255) // 256, dtype=torch.int32, device=self.device)
        self.half = 0
        self.pushes = 0

    # -----------------------------------------------------------------------------------------------------------------
    def _info0(self, info, first_key_column):
        """Address of the column of the simulators' info block that holds ``goal_met`` / ``reached`` and the block's
        leading dimension; the violations and the safety cost are the two columns behind it."""
        n = self.n
        if isinstance(first_key_column, bool) or not isinstance(first_key_column, (int, np.integer)) or first_key_column < 0:
            raise ValueError("EpisodeLedger.push: first_key_column is a column index (got %r)" % (first_key_column,))
        if isinstance(info, dict):                    # what ``envs.device`` returns: three column views of one block
            cols = list(info.values())
            want = ("num_safety_violation", "safety_cost")
            if len(cols) != 3 or tuple(info)[1:] != want:
                raise ValueError("EpisodeLedger.push: an info dict holds goal_met / reached, %s and %s, in this order" % want)
            for x in cols:
                self._is(x, "info", 8, True)
            ld = cols[0].stride(0) if n > 1 else 3
            ok = all(x.dim() == 1 and x.shape[0] == n and (n == 1 or x.stride(0) == ld) for x in cols)
            if not ok or ld < 3 or any(x.data_ptr() != cols[0].data_ptr() + 8 * j for j, x in enumerate(cols)):
                raise ValueError("EpisodeLedger.push: the info dict's tensors must be the columns of one float64 (%d, 3) "
                                 "block" % n)
            if first_key_column != 0:
                raise ValueError("EpisodeLedger.push: first_key_column goes with an info tensor, not with a dict")
            return cols[0], cols[0].data_ptr(), int(ld)
        self._is(info, "info", 8, True)
        if info.dim() != 2 or info.shape[0] != n or info.shape[1] < first_key_column + 3 or info.stride(1) != 1 or \
                (n > 1 and info.stride(0) < info.shape[1]):
            raise ValueError("EpisodeLedger.push: info must be a float64 (%d, >= %d) tensor with unit column stride"
                             % (n, first_key_column + 3))
        return info, info.data_ptr() + 8 * int(first_key_column), int(info.stride(0)) if n > 1 else int(info.shape[1])

    def _is(self, x, name, itemsize, floating):
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype.itemsize != itemsize or x.dtype.is_floating_point != floating or \
                x.dtype == torch.bool or x.dtype.is_complex:
            raise ValueError("EpisodeLedger.push: %s must be a %s tensor" % (name, {(8, True): "float64", (4, False): "int32"}[
                (itemsize, floating)]))
        if x.device != self._fin.device:
            raise ValueError("EpisodeLedger.push: %s lives on %s, the ledger on %s" % (name, x.device, self._fin.device))

    def push(self, reward, done, info, ep_step, max_episode_steps, *, first_key_column=0, flags=None, vstep, updates):
        """One vector step: ``reward`` (n,) float64, ``done`` / ``ep_step`` (n,) int32 and ``info`` as the device
        simulators return them (the dict of ``envs.device``, or a float64 (n, >= 3) block whose columns
        ``first_key_column``, + 1, + 2 are ``goal_met`` / ``reached``, ``num_safety_violation``, ``safety_cost``);
        ``flags``: (n,) bool / uint8, set where the backup controller decided the step (None: it never acts);
        ``vstep`` / ``updates``: the vector step's index and the driver's update count, stamped on the records of the
        episodes that end in this step.  Two launches, no host read, no allocation."""
        import torch
        n = self.n
        for name, x, size, fl in (("reward", reward, 8, True), ("done", done, 4, False), ("ep_step", ep_step, 4, False)):
            self._is(x, name, size, fl)
            if x.dim() != 1 or x.shape[0] != n or not x.is_contiguous():
                raise ValueError("EpisodeLedger.push: %s must be a contiguous (%d,) tensor (got %s)" % (name, n, tuple(x.shape)))
        _, info0, info_ld = self._info0(info, first_key_column)
        if flags is not None:
            if not isinstance(flags, torch.Tensor) or flags.dtype not in (torch.bool, torch.uint8) or flags.dim() != 1 or \
                    flags.shape[0] != n or not flags.is_contiguous() or flags.device != self._fin.device:
                raise ValueError("EpisodeLedger.push: flags must be a contiguous (%d,) bool / uint8 tensor on %s"
                                 % (n, self._fin.device))
        for name, v, lo in (("max_episode_steps", max_episode_steps, 1), ("vstep", vstep, 0), ("updates", updates, 0)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
                raise ValueError("EpisodeLedger.push: %s must be an int in [%d, 2^31) (got %r)" % (name, lo, v))
        if self._fin.device.type != "cuda":
            raise ValueError("EpisodeLedger.push: the ledger's kernels run on a CUDA / HIP device, this one lives on %s"
                             % self._fin.device)
        from .arena import stream_ptr
        s = stream_ptr()
        _lib.call("nlbac_episode_step", n, reward.data_ptr(), info0, info_ld, done.data_ptr(), ep_step.data_ptr(),
                  int(max_episode_steps), None if flags is None else flags.data_ptr(), self._dstate.data_ptr(),
                  self._istate.data_ptr(), self._fin.data_ptr(), self._counts.data_ptr(), s)
        half = self.half
        _lib.call("nlbac_episode_append", n, self._fin.data_ptr(), self._counts.data_ptr(), self._dstate.data_ptr(),
                  self._istate.data_ptr(), self._ring.data_ptr(), self.capacity, self.head.data_ptr(), half, int(vstep),
                  int(updates), s)
        self.half = 1 - half
        self.pushes += 1

    # -----------------------------------------------------------------------------------------------------------------
    def arrays(self, since=0):
        """The records ``since .. total - 1`` of the log, in log order — vector step by vector step, lane order within
        one — as a dict of numpy arrays (``HISTORY_KEYS``, ``vstep``, ``info0``, and ``total``: records ever written).
        One device-to-host copy.  Raises ``ValueError`` when ``since`` points at records the ring (``capacity``) has
        overwritten."""
        if isinstance(since, bool) or not isinstance(since, (int, np.integer)) or since < 0:
            raise ValueError("EpisodeLedger.records: since is a record index (got %r)" % (since,))
        host = self._log.cpu().numpy()
        pos, total = (int(v) for v in host[2 * self.half:2 * self.half + 2])
        if since > total:
            raise ValueError("EpisodeLedger.records: since = %d, the log holds %d records" % (since, total))
        if total - since > self.capacity:
            raise ValueError("EpisodeLedger.records: records %d .. %d have been overwritten — the ring's capacity is %d "
                             "records and %d were written; read more often or construct the ledger with a larger capacity"
                             % (since, total - self.capacity - 1, self.capacity, total))
        ring = host[_HEAD_WORDS:].view(RECORD_DTYPE)
        assert pos == total % self.capacity
        rec = ring[np.arange(since, total) % self.capacity]
        return dict(episode=np.arange(since, total, dtype=np.int64), reward=rec["ret"].copy(),
                    length=rec["length"].astype(np.int64), violations=rec["violations"].astype(np.int64),
                    safety_cost=rec["safety_cost"].copy(), goal_met=(rec["info0"] != 0).astype(np.int64),
                    timeout=rec["timeout"].astype(np.int64), lane=rec["lane"].astype(np.int64),
                    lane_episode=rec["lane_episode"].astype(np.int64),
                    total_steps=(rec["vstep"].astype(np.int64) + 1) * self.n, updates=rec["updates"].astype(np.int64),
                    backup_steps=rec["backup_steps"].astype(np.int64), vstep=rec["vstep"].astype(np.int64),
                    info0=rec["info0"].copy(), total=total)

    def records(self, since=0):
        """``(arrays, history)``: ``arrays(since)`` and the same as a list of dicts, ``train.train``'s shape."""
        arrays = self.arrays(since)
        return arrays, history_of(arrays)

    def totals(self):
        """Sums over all lanes (float64, on the host, one small copy): ``episodes``, ``reward``, ``violations``,
        ``safety_cost``, ``steps`` and ``backup_steps`` of the finished episodes, and the same of the episodes still
        running as ``open_*``."""
        n = self.n
        host = self._state.cpu().numpy()
        d = host[:_lib.EPISODE_DSTATE * n].view(np.float64).reshape(_lib.EPISODE_DSTATE, n)
        i = host[_lib.EPISODE_DSTATE * n:].view(np.int32)[:_lib.EPISODE_ISTATE * n].reshape(_lib.EPISODE_ISTATE, n).astype(np.int64)
        return dict(episodes=int(i[4].sum()), reward=float(d[3].sum()), safety_cost=float(d[4].sum()),
                    violations=int(d[5].sum()), steps=int(i[2].sum()), backup_steps=int(i[3].sum()),
                    open_reward=float(d[0].sum()), open_safety_cost=float(d[1].sum()), open_violations=int(d[2].sum()),
                    open_steps=int(i[0].sum()), open_backup_steps=int(i[1].sum()))


def ledger_for(episodes, n, device):
    """The ``episodes=`` argument of the drivers: True (default capacity), an int (capacity) or an ``EpisodeLedger`` of
    ``n`` lanes.  Every check before anything touches a device."""
    if isinstance(episodes, EpisodeLedger):
        if episodes.n != n:
            raise ValueError("episodes=: the ledger has %d lanes, the environment %d" % (episodes.n, n))
        return episodes
    if episodes is True:
        return EpisodeLedger(n, device)
    if isinstance(episodes, (int, np.integer)) and not isinstance(episodes, bool):
        return EpisodeLedger(n, device, capacity=int(episodes))
    raise ValueError("episodes= is None / False, True, a capacity (int) or an EpisodeLedger (got %r)" % (episodes,))


def write_tsv(path, history):
    """One tab-separated line per record under a header line (``HISTORY_KEYS``)."""
    with open(path, "w") as f:
        f.write("\t".join(HISTORY_KEYS) + "\n")
        for rec in history:
            f.write("\t".join("%.17g" % rec[k] if isinstance(rec[k], float) else "%d" % rec[k] for k in HISTORY_KEYS) + "\n")
