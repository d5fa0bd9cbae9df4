"""Host side of the dopri5 control-block protocol: how the host learns the step-size controller's decision.

Where the controller launch writes the pinned control block itself, the host polls the block's stamp (a sequence lock
the launch writes, nlbac_rk_chain::ctl_seq); where it cannot (data parallelism, the host-driven steps of ragged row
counts), the block is copied on a side stream behind an event (``post``).  ``ControlBlockReader`` owns both ways: the
side stream, the event pair, the pinned blocks by problem count and the stamp counter.  What belongs to ONE solve — the
pending read and the solve's stamp range — is kept in that solve's ``ctx`` (keys ``ctl_pending`` / ``ctl_seq``, touched
here only): an owner of captured hipGraphs swaps solves by swapping ``ctx``, and a replayed solve has nothing pending.
The device block itself is a scratch buffer of the solver (``_ctl``).
"""
import time

import torch

from . import _lib
from .ode_consts import CTL_DONE, CTL_SEQ


class ControlBlockReader:
    # One stamp counter per process: solvers share pinned blocks (a solver's per-problem children read through their
    # parent's reader), and a stamp must never repeat within a block.
    _seq = [0]

    def __init__(self, device, stats):
        self.device = device
        self.stats = stats         # the owning solver's counters (``poll_drained``)
        self.side = None           # the read-back stream and its events: created on first use
        self.events = None
        self.pin = {}              # problems -> pinned (P, DOPRI_CTL) float64 block

    def io(self, P):
        """(side stream, pinned block for P problems), created on first use."""
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.device)
            self.events = (torch.cuda.Event(), torch.cuda.Event())
        pin = self.pin.get(P)
        if pin is None:
            pin = self.pin[P] = torch.zeros(P, _lib.DOPRI_CTL, dtype=torch.float64).pin_memory()
        return self.side, pin

    def begin(self, ctx):
        """The stamps of a solve's controller launches start here (``next_stamp``)."""
        ctx["ctl_seq"] = None

    def post(self, ctx, P, src):
        """After an attempted step: send the device control block ``src`` to pinned host memory on a side stream, so
        that the host can read the accept decision as soon as the controller has run — without draining the launch
        stream, on which the caller may have queued independent work behind the attempt (the agent queues its
        whole critic phase there).  Not inside a hipGraph capture (the replay path reads the device block)."""
        if torch.cuda.is_current_stream_capturing():
            return
        side, pin = self.io(P)
        ctx["ctl_seq"] = None        # (a copy, read behind its event: nothing to poll)
        ev_a, ev_b = self.events
        ev_a.record()
        side.wait_event(ev_a)
        with torch.cuda.stream(side):
            pin.copy_(src, non_blocking=True)
            ev_b.record()
        ctx["ctl_pending"] = P

    def posted(self, ctx, P):
        """Device-driven chain: the controller launches have written the host's copy themselves (``ctl_host``); mark the
        point on the launch stream behind which it is complete."""
        if torch.cuda.is_current_stream_capturing():
            return
        self.io(P)
        if ctx.get("ctl_seq") is None:
            self.events[1].record()     # (stamped blocks are polled: no event, no marker on the launch stream)
        ctx["ctl_pending"] = P

    def next_stamp(self, ctx):
        """Stamp for the next controller launch that writes the host's copy; ctx["ctl_seq"] = (stamp of the solve's first
        such launch, stamp of its latest).  None when the block is read behind an event."""
        if torch.cuda.is_current_stream_capturing():
            ctx["ctl_seq"] = None
            return 0.0
        seq = self._seq
        seq[0] += 1
        rng = ctx.get("ctl_seq")
        ctx["ctl_seq"] = (seq[0] if rng is None else rng[0], seq[0])
        return float(seq[0])

    def poll(self, P, first, last, patience=0.05):
        """Wait for the stamped control blocks of the launch with stamp ``last``: a problem's block is complete when it
        carries that stamp — or an earlier one of the same solve with the done flag (launches skip finished problems).
        Sequence-lock read: stamp, block, stamp.  After ``patience`` seconds of spinning the launch stream is drained
        (everything queued has then run) and the block must be there."""
        arr = self.pin[P].numpy()          # (the same memory)
        t0 = drained = None
        n = 0
        stamps = arr[:, CTL_SEQ]
        while True:
            s1 = stamps.tolist()                       # (stamp, block, stamp: the sequence lock's read side)
            if all(x == last or first <= x < last for x in s1):
                c = arr.copy()
                if all(c[p, CTL_SEQ] == s1[p] and (s1[p] == last or c[p, CTL_DONE] > 0) for p in range(P)):
                    return torch.from_numpy(c)
            n += 1
            if n & 63 == 0:
                now = time.perf_counter()
                if t0 is None:
                    t0 = now
                elif drained:
                    raise _lib.NlbacError("control block %r never reached stamp %d (solve from %d)" % (s1, last, first))
                elif now - t0 > patience:
                    torch.cuda.current_stream().synchronize()
                    drained = True
                    self.stats["poll_drained"] = self.stats.get("poll_drained", 0) + 1

    def read(self, ctx, P, before_wait=None):
        """Host copy of the control block of the last attempted step, if one was posted for ``P`` problems (consumed);
        None otherwise — the caller then reads the device block.  ``before_wait``: the owner's hook, run before the
        host blocks (it queues independent work behind the attempt)."""
        if ctx.pop("ctl_pending", None) != P:
            return None
        if before_wait is not None:
            before_wait()
        rng = ctx.get("ctl_seq")
        if rng is not None:
            return self.poll(P, *rng)
        self.events[1].synchronize()
        return self.pin[P].clone()
