"""``rollout(m, x0, controls, dt, method="dopri5")`` of the Unicycle NODE under its two step controls, each against itself
across rounds (their results differ by design: one error norm per 32-row tile against one for the batch):

  tile   ``step_control="tile"``: the whole horizon in one ``nlbac_node_dopri_tile_fwd`` launch, its backward in one
         ``nlbac_node_dopri_tile_bwd`` (+ the weight-gradient launch over the used slots);
  batch  ``step_control="batch"`` (the default): H chained solves — per solve the f0 launch, the probe, the attempts and
         their controller launches, and a look by the host at the control block.

Two regimes: ``single`` — dt = 0.02 on the untrained net, one accepted step per interval; ``multi`` — dt = 0.5 with x0 and
the controls scaled by (0.05, 1, 20) tile after tile, several steps per interval and tiles that need different numbers
of them.  rows x H x {forward only, + gradients w.r.t. x0 and the controls, + parameter gradients}.

One process, alternating rounds, timed with device events after warm-up.

    python tools/rollout_tile_vs_chain.py [--rounds 7] [--reps 3] [--out profiles/rollout_dopri_tile_vs_chain.txt]

Columns: median over the rounds of the mean time of ``reps`` solves (us), the ratio batch / tile, library calls per solve
(the weight refresh included), each path's spread (max - min over the rounds), and of the tile path the accepted steps
per tile over the horizon — mean, max and max / mean: the work a batch-wide control would make every tile do is the
max.  ``max_steps`` is what the largest tile needs (read from a first run without gradients); a row whose kept buffers
would pass ``--keep-gb`` is left out and says so.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib  # noqa: E402
from nlbac_amd import rollout as R  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

PATHS = ("tile", "batch")
REGIMES = {"single": (0.02, (1.0,)), "multi": (0.5, (0.05, 1.0, 20.0))}


def run(path, m, x0, c, dt, mode, w, max_steps, info=None):
    kw = dict(step_control="tile", max_steps=max_steps, info=info) if path == "tile" else {}
    if mode == "fwd":
        with torch.no_grad():
            return R.rollout(m, x0, c, dt, method="dopri5", **kw)
    x, u = x0.detach().requires_grad_(), c.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    out = R.rollout(m, x, u, dt, method="dopri5", **kw)
    (out * w).sum().backward()
    return out


def kept_bytes(m, mode, max_steps, B):
    """What the tile path keeps (forward and backward), from the docstring of ``rollout``."""
    ng, ns, hid = m.n_s * m.n_u, m.n_s, 100
    per = {"fwd": 0, "inputs": 7 * (4 * ng + 112), "params": 7 * (8 * ng + 8 * ns + 56 * hid + 112)}[mode]
    return per * max_steps * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 8192, 32768])
    ap.add_argument("--horizons", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--keep-gb", type=float, default=16.0)
    ap.add_argument("--out", default=os.path.join("profiles", "rollout_dopri_tile_vs_chain.txt"))
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
    ns, nu = m.n_s, m.n_u
    say("rollout(method='dopri5') of the Unicycle NODE: step_control='tile' (one launch each way) against 'batch' (chained solves)")
    say("%s, rounds %d x reps %d, medians in us" % (torch.cuda.get_device_name(0), a.rounds, a.reps))
    say("%-6s %6s %3s %-7s | %10s %10s %8s | %5s %6s | %8s %8s | %6s %4s %5s | %5s" % (
        "regime", "rows", "H", "mode", "tile us", "batch us", "batch/1", "l_til", "l_bat", "sp_tile", "sp_batch",
        "acc_mu", "max", "ratio", "slots"))
    for regime, (dt, scale) in REGIMES.items():
        for B in a.rows:
            for H in a.horizons:
                g = torch.Generator(device="cuda").manual_seed(1)
                x0 = torch.rand(B, ns, device="cuda", generator=g) * 2 - 1
                c = torch.rand(H, B, nu, device="cuda", generator=g) * 2 - 1
                w = torch.randn(H + 1, B, ns, device="cuda", generator=g)
                for j, lo in enumerate(range(0, B, 32)):
                    x0[lo:lo + 32] *= scale[j % len(scale)]
                    c[:, lo:lo + 32] *= scale[j % len(scale)]
                info = {}
                run("tile", m, x0, c, dt, "fwd", w, None, info)
                acc = info["accepted"].sum(1).float()
                assert int(info["status"].abs().max()) == 0
                mu, mx = float(acc.mean()), int(acc.max())
                for mode in ("fwd", "inputs", "params"):
                    for p in m.parameters():
                        p.requires_grad_(mode == "params")
                        p.grad = None
                    gb = kept_bytes(m, mode, mx, B) / 2 ** 30
                    if gb > a.keep_gb:
                        say("%-6s %6d %3d %-7s | left out: %d slots x 7 stages x %d rows keep %.0f GB (every tile gets the "
                            "largest tile's slots)" % (regime, B, H, mode, mx, B, gb))
                        continue
                    launches = {}
                    for path in PATHS:                  # warm-up, library calls per solve
                        run(path, m, x0, c, dt, mode, w, mx)
                        torch.cuda.synchronize()
                        del calls[:]
                        run(path, m, x0, c, dt, mode, w, mx)
                        torch.cuda.synchronize()
                        launches[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                    tm = {p: [] for p in PATHS}
                    for _ in range(a.rounds):
                        for path in PATHS:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(a.reps):
                                run(path, m, x0, c, dt, mode, w, mx)
                            e1.record()
                            e1.synchronize()
                            tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                    med = {p: statistics.median(v) for p, v in tm.items()}
                    say("%-6s %6d %3d %-7s | %10.1f %10.1f %8.2f | %5d %6d | %8.1f %8.1f | %6.2f %4d %5.2f | %5d" % (
                        regime, B, H, mode, med["tile"], med["batch"], med["batch"] / med["tile"], launches["tile"],
                        launches["batch"], max(tm["tile"]) - min(tm["tile"]), max(tm["batch"]) - min(tm["batch"]),
                        mu, mx, mx / mu, mx))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
