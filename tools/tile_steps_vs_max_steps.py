"""``odeint_dense(m, y0, t, step_control="tile")`` of the Unicycle NODE with the step slots counted per tile
(``tile_steps=``) against one count for every tile (``max_steps=``), in ``tools/odeint_dense_tile_vs_batch.py``'s
``multi`` regime: the nine points 0 .. 1.47, inputs scaled by (0.05, 1, 5) tile after tile, so that the tiles need
different numbers of steps.  rows x {gradients w.r.t. y0, + parameter gradients} x three ways to size the slots:

  max     ``max_steps`` = the largest count any tile takes (the least the call admits): [slot][stage][row] over
          max * 7 * B rows, zero-filled for every tile that takes fewer;
  exact   ``tile_steps`` = every tile's own count (``info["slots"]`` of a ``"count"`` run in the same keep mode): pages of
          7 stages x 32 rows, sum(counts) of them;
  count   ``tile_steps="count"``: the forward launch once with nothing kept, the counts to the host, then ``exact``.

All three give the same values and input gradients bit for bit (``tests/test_tile_steps_gpu.py``); ``max`` is the
reference — the call as it was before ``tile_steps``.  One process, alternating rounds, device events after a warm-up.

    python tools/tile_steps_vs_max_steps.py [--rounds 5] [--rows 256 8192 32768] [--out profiles/tile_steps_vs_max_steps.txt]

Columns: the pages kept against max * n_tiles and their ratio (what the step counts promise), the peak of allocated
device memory over forward + backward (GB) and its ratio to ``max``'s, the medians of the forward and of forward +
backward (us) with their ratio to ``max``'s, and the spread (max - min over the rounds) of forward + backward.  Where
the library refuses the ``max`` call (the weight-gradient launch takes at most 2^29 elements per layer) or its buffers
would pass ``--keep-gb``, the row says so and the other two stand without a ratio.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import ode_dense  # noqa: E402
from nlbac_amd._lib import NlbacError  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402
from odeint_dense_tile_vs_batch import inputs, kept_bytes  # noqa: E402

VARIANTS = ("max", "exact", "count")


def solve(m, y0, t, w, kw):
    """One forward and backward; returns their device times (us) and the peak of allocated memory (bytes)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    y = y0.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    e[0].record()
    out = ode_dense.odeint_dense(m, y, t, step_control="tile", **kw)
    e[1].record()
    (out * w).sum().backward()
    e[2].record()
    e[2].synchronize()
    return e[0].elapsed_time(e[1]) * 1e3, e[0].elapsed_time(e[2]) * 1e3, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 8192, 32768])
    ap.add_argument("--keep-gb", type=float, default=64.0)
    ap.add_argument("--out", default=os.path.join("profiles", "tile_steps_vs_max_steps.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6)
    say("odeint_dense(step_control='tile') of the Unicycle NODE, multi-step regime: slots per tile (tile_steps) against "
        "max_steps")
    say("%s, %d alternating rounds, medians in us; reference: max_steps = the largest tile's count" % (
        torch.cuda.get_device_name(0), a.rounds))
    say("%6s %-7s %-6s | %7s %8s %6s | %8s %6s | %10s %6s | %10s %6s %8s | %s" % (
        "rows", "mode", "slots", "pages", "max*til", "ratio", "peak GB", "/max", "fwd us", "/max", "f+b us", "/max", "spread",
        "accepted per tile: mean / max"))
    for B in a.rows:
        y0, t = inputs("multi", B)
        w = torch.randn(len(t), B, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        for mode in ("inputs", "params"):
            for p in m.parameters():
                p.requires_grad_(mode == "params")
            info = {}
            solve(m, y0, t, w, dict(tile_steps="count", info=info))
            assert int(info["status"].abs().max()) == 0
            counts = info["slots"]
            tiles, mx, pages = len(counts), int(counts.max()), int(counts.sum())
            kws = {"max": dict(max_steps=mx), "exact": dict(tile_steps=counts), "count": dict(tile_steps="count")}
            variants = list(VARIANTS)
            gb = kept_bytes(m, mode, mx, B) / 2 ** 30
            if gb > a.keep_gb:
                say("%6d %-7s max    | left out: max_steps = %d keeps %.0f GB" % (B, mode, mx, gb))
                variants.remove("max")
            for v in list(variants):                # warm-up: the allocator's blocks, the workspaces
                try:
                    solve(m, y0, t, w, kws[v])
                except NlbacError as e:
                    if v != "max":
                        raise
                    say("%6d %-7s max    | refused with max_steps = %d (%d pages): %s" % (B, mode, mx, mx * tiles, e))
                    variants.remove("max")
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
            tm = {v: [] for v in variants}
            for _ in range(a.rounds):
                for v in variants:
                    tm[v].append(solve(m, y0, t, w, kws[v]))
            med = {v: [statistics.median(r[i] for r in tm[v]) for i in range(3)] for v in variants}
            ref = med.get("max", [float("nan")] * 3)
            for v in variants:
                kept = mx * tiles if v == "max" else pages
                fb = [r[1] for r in tm[v]]
                say("%6d %-7s %-6s | %7d %8d %6.2f | %8.3f %6.2f | %10.1f %6.2f | %10.1f %6.2f %8.1f | %.2f / %d" % (
                    B, mode, v, kept, mx * tiles, kept / (mx * tiles), med[v][2] / 2 ** 30, med[v][2] / ref[2],
                    med[v][0], med[v][0] / ref[0], med[v][1], med[v][1] / ref[1], max(fb) - min(fb),
                    float(counts.float().mean()), mx))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
