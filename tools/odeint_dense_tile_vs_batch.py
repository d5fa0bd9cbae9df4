"""``odeint_dense(m, y0, t)`` of the Unicycle NODE under its two step controls, each against itself across rounds (their
results differ by design: one error norm per 32-row tile against one for the batch):

  tile   ``step_control="tile"``: the whole time series in one ``nlbac_node_dopri_tile_dense_fwd`` launch, its backward in
         one ``nlbac_node_dopri_tile_dense_bwd`` (+ the weight-gradient launch over the used slots);
  batch  ``step_control="batch"`` (the default): the device-driven chain — the f0 launch, the probe, the attempts and their
         controller launches, a look by the host at the control block — then ``nlbac_dopri_dense_fwd`` over the slots;
         backward ``nlbac_dopri_dense_bwd``, then a step backward per accepted step and a carry launch per boundary.

Two regimes: ``grid17`` — ``tools/odeint_dense_probe.py``'s grid, T = 17 points over [0, 0.32], inputs uniform in [-1, 1];
``multi`` — the nine points 0 .. 1.47 of ``tests/test_odeint_dense_tile_gpu.py`` with inputs of its recipe (x in
[-2, 2]^2 x [-3, 3], u in [-3.5, 3.5] x [-12, 12]) scaled by (0.05, 1, 5) tile after tile: tiles that need different
numbers of steps.  rows x {forward only, + gradients w.r.t. y0, + parameter gradients}.

One process, alternating rounds, timed with device events after warm-up.

    python tools/odeint_dense_tile_vs_batch.py [--rounds 7] [--reps 3] [--out profiles/odeint_dense_tile_vs_batch.txt]

Columns: median over the rounds of the mean time of ``reps`` solves (us), the ratio batch / tile, library calls per solve
(the weight refresh included), each path's spread (max - min over the rounds), the accepted steps of the batch-wide
solve, and of the tile path the accepted steps per tile — mean, max and max / mean — and the slots per tile.
``max_steps`` is what the largest tile needs in a first run without gradients plus ``SLACK``: a solve that keeps mask
words only sums f_net's output layer in two parts, its values differ from the other modes' in the last bits, and a tile
with an error ratio at the accept threshold then takes a step more or less.  A row whose kept buffers would pass
``--keep-gb`` is left out and says so.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib  # noqa: E402
from nlbac_amd import ode_dense  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

PATHS = ("tile", "batch")
SLACK = 4
MULTI_GRID = [0.0, 0.01, 0.02, 0.05, 0.3, 0.35, 0.4, 0.6, 1.47]


def inputs(regime, B):
    g = torch.Generator(device="cuda").manual_seed(1)
    if regime == "grid17":
        return torch.rand(B, 5, device="cuda", generator=g) * 2 - 1, torch.linspace(0.0, 0.32, 17)
    lim = torch.tensor([2.0, 2.0, 3.0, 3.5, 12.0], device="cuda")
    y0 = (torch.rand(B, 5, device="cuda", generator=g) * 2 - 1) * lim
    for j, lo in enumerate(range(0, B, 32)):
        y0[lo:lo + 32] *= (0.05, 1.0, 5.0)[j % 3]
    return y0, torch.tensor(MULTI_GRID)


def run(path, m, y0, t, mode, w, max_steps, info=None):
    kw = dict(step_control="tile", max_steps=max_steps, info=info) if path == "tile" else {}
    if mode == "fwd":
        with torch.no_grad():
            return ode_dense.odeint_dense(m, y0, t, **kw)
    y = y0.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    out = ode_dense.odeint_dense(m, y, t, **kw)
    (out * w).sum().backward()
    return out


def kept_bytes(m, mode, max_steps, B):
    """What the tile path keeps (forward and backward): ``rollout``'s figures per (slot, stage, row)."""
    ng, ns, hid = m.n_s * m.n_u, m.n_s, 100
    per = {"fwd": 0, "inputs": 7 * (4 * ng + 112), "params": 7 * (8 * ng + 8 * ns + 56 * hid + 112)}[mode]
    return per * max_steps * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 8192, 32768])
    ap.add_argument("--keep-gb", type=float, default=16.0)
    ap.add_argument("--out", default=os.path.join("profiles", "odeint_dense_tile_vs_batch.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    calls = []
    real = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6)
    say("odeint_dense of the Unicycle NODE: step_control='tile' (one launch each way) against 'batch' (chain + slot walk)")
    say("%s, rounds %d x reps %d, medians in us" % (torch.cuda.get_device_name(0), a.rounds, a.reps))
    say("%-6s %6s %2s %-7s | %10s %10s %8s | %5s %6s | %8s %8s | %5s | %6s %4s %5s | %5s" % (
        "regime", "rows", "T", "mode", "tile us", "batch us", "batch/1", "l_til", "l_bat", "sp_tile", "sp_batch", "s_bat",
        "acc_mu", "max", "ratio", "slots"))
    for regime in ("grid17", "multi"):
        for B in a.rows:
            y0, t = inputs(regime, B)
            w = torch.randn(len(t), B, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
            info = {}
            run("tile", m, y0, t, "fwd", w, None, info)
            acc = info["accepted"].float()
            assert int(info["status"].abs().max()) == 0
            mu, mx = float(acc.mean()), int(acc.max())
            slots = mx + SLACK
            for mode in ("fwd", "inputs", "params"):
                for p in m.parameters():
                    p.requires_grad_(mode == "params")
                    p.grad = None
                gb = kept_bytes(m, mode, slots, B) / 2 ** 30
                if gb > a.keep_gb:
                    say("%-6s %6d %2d %-7s | left out: %d slots x 7 stages x %d rows keep %.0f GB (every tile gets the "
                        "largest tile's slots)" % (regime, B, len(t), mode, slots, B, gb))
                    continue
                launches = {}
                for path in PATHS:                  # warm-up, library calls per solve
                    run(path, m, y0, t, mode, w, slots)
                    torch.cuda.synchronize()
                    del calls[:]
                    run(path, m, y0, t, mode, w, slots)
                    torch.cuda.synchronize()
                    launches[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                keep = {"fwd": "none", "inputs": "inputs", "params": "params"}[mode]
                s_batch = len(ode_dense.solver_of(m, keep).ctx["steps"])
                tm = {p: [] for p in PATHS}
                for _ in range(a.rounds):
                    for path in PATHS:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.reps):
                            run(path, m, y0, t, mode, w, slots)
                        e1.record()
                        e1.synchronize()
                        tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                med = {p: statistics.median(v) for p, v in tm.items()}
                say("%-6s %6d %2d %-7s | %10.1f %10.1f %8.2f | %5d %6d | %8.1f %8.1f | %5d | %6.2f %4d %5.2f | %5d" % (
                    regime, B, len(t), mode, med["tile"], med["batch"], med["batch"] / med["tile"], launches["tile"],
                    launches["batch"], max(tm["tile"]) - min(tm["tile"]), max(tm["batch"]) - min(tm["batch"]), s_batch,
                    mu, mx, mx / mu, slots))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
