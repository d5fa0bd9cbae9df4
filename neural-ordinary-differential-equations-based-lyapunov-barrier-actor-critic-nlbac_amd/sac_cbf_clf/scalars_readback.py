"""Host side of the scalars read-back: how the 512-byte device scalars block (``_layout.py``: losses, temperatures,
multipliers) reaches the host.  Two ways, as for the solvers' control block (``ode_ctl.ControlBlockReader``): the
update's last launch — the actors' optimiser step — writes the block to pinned memory itself (``nlbac_adam_fused``'s
mirror arguments: no copy launch between that step and the host's wait), or the block is copied behind the launch
stream.  ``ScalarsReadback`` owns the three pinned blocks (0: this update's; 1, 2: alternating, for ``"lagged"``
callers), their events, which block the current update mirrors to and which one the last optimiser step has written.
"""
import torch

from . import _layout as SC


class ScalarsReadback:
    def __init__(self, sc):
        self.sc = sc                 # the device block
        self.pin = [torch.zeros(SC.SC_SIZE, dtype=torch.float32).pin_memory() for _ in range(3)]
        self.ev = [torch.cuda.Event() for _ in range(3)]
        self.lag = None              # block of the previous "lagged" call, still on its way or unread
        self.flip = 0                # the "lagged" block used last (1 or 2)
        self.mirror = None           # (block index, pinned block) the current update's last optimiser step writes to
        self.mirror_done = None      # block index that step HAS written to since the last ``returns``

    def read(self):
        """Host copy of the device scalars (one 512-byte read through a pinned buffer; waits for the launch stream)."""
        self.pin[0].copy_(self.sc, non_blocking=True)
        self.ev[0].record()
        self.ev[0].synchronize()
        return self.pin[0].numpy().copy()

    def choose_mirror(self, sync, direct):
        """Start of an update: where its last launch leaves the scalars block for the host — straight in pinned memory
        when the caller wants values (``sync``) and ``direct`` holds: not under hipGraph replay (the address would be
        baked in) or data parallelism (the step is not the last thing that happens)."""
        self.mirror = None
        if sync and direct:
            k = 0
            if sync == "lagged":
                k = self.flip = 1 + (self.flip & 1)
            self.mirror = (k, self.pin[k])

    def mirrored(self, k):
        """The last optimiser step, which writes block ``k``, has been queued.  (The event is recorded here, not in
        ``returns``: what the update queues behind that step for its successor is not waited for.)"""
        self.mirror_done = k
        self.ev[k].record()

    def returns(self, sync):
        """The scalars block as an update returns it.  ``sync``: True — of this update (the host waits for it, as the
        reference's ``.item()`` calls do); "lagged" — of the previous ``"lagged"`` call (None on the first), while this
        update's are on their way to pinned memory: the launch stream never drains, for drivers that only log the
        values; False — nothing."""
        if not sync:
            return None
        mirrored, self.mirror_done = self.mirror_done, None
        if sync == "lagged":
            if mirrored is not None:
                k = mirrored
            else:
                k = self.flip = 1 + (self.flip & 1)
                self.pin[k].copy_(self.sc, non_blocking=True)
            prev, self.lag = self.lag, k
            if mirrored is None:
                self.ev[k].record()
            if prev is None:
                return None
            self.ev[prev].synchronize()
            return self.pin[prev].numpy().copy()
        if mirrored is not None:
            self.ev[mirrored].synchronize()
            return self.pin[mirrored].numpy().copy()
        return self.read()
