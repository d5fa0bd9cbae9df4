"""Time of one NODE validation (``SAC_CBF_CLF.validate_node``) beside one NODE fit on the same windows
(``SAC_CBF_CLF.fit_node_windows``), and of the statistics launches on their own.

    python tools/node_validation_cost.py [--windows 4096] [--horizon 8] [--runs 5] [--reps 5]

Unicycle (euler, dopri5) and SimulatedCars (rk4).  The replay holds 32768 synthetic transitions in episodes of 200 steps
(chained observations, so most windows are valid; ``tools/fit_windows_probe.py`` fills its replay the same way).  Every
time is the median over ``runs`` of the mean of ``reps`` calls between two device events, after a warm-up:

  validate   ``validate_node(memory, W, horizon=H)`` — the draw of W start rows on the host and their upload, the window
             gather, the state / target rows, one no-grad solve over the H intervals, ``nlbac_traj_err_stats``
  windows    ``validate_node_windows(rows, valid)`` on windows already gathered
  stats      the two launches of ``nlbac_traj_err_stats`` alone
  fit        ``fit_node_windows(rows, valid, counts)`` on the same windows (forward, loss, backward, weight gradients,
             Adam): what a validation is to be held against

dopri5 is the chained solve: every interval waits for the host's look at its step control, in the validation as in
the fit.  No bar hangs on these numbers."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fit_windows_probe import fill, make_agent  # noqa: E402
from nlbac_amd.node_fit import traj_error_stats_launch  # noqa: E402


def timed(fn, runs, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    W, H = a.windows, a.horizon
    print("%-14s %-6s %5s %2s | %21s | %10s %9s | %21s | %8s %6s" % (
        "env", "solver", "W", "H", "validate us (min-max)", "windows us", "stats us", "fit us (min-max)", "val/fit", "valid"))
    for env_name, solver in (("Unicycle", "euler"), ("Unicycle", "dopri5"), ("SimulatedCars", "rk4")):
        agent, env = make_agent(env_name, solver)
        mem = fill(agent, env_name, env, 32768)
        ns = agent.task.n_s
        val = timed(lambda: agent.validate_node(mem, W, horizon=H, stride=1), a.runs, a.reps)
        starts = torch.randint(0, len(mem), (W,), generator=torch.Generator().manual_seed(H))
        rows, valid = mem.sample_windows(W, H, idx=starts)
        counts = mem.window_counts
        win = timed(lambda: agent.validate_node_windows(rows, valid), a.runs, a.reps)
        w = agent._validate_ws(W, H)
        stats = torch.empty(5, H, ns, dtype=torch.float64, device="cuda")
        nvalid = torch.empty((), dtype=torch.int64, device="cuda")
        st = timed(lambda: traj_error_stats_launch(w["xs"], w["target"], w["x0"], valid, H, W, ns, w["scratch"], stats, nvalid),
                   a.runs, a.reps)
        fit = timed(lambda: agent.fit_node_windows(rows, valid, counts), a.runs, a.reps)
        print("%-14s %-6s %5d %2d | %8.1f (%5.1f-%5.1f) | %10.1f %9.1f | %8.1f (%5.1f-%5.1f) | %8.2f %6.3f" % (
            env_name, solver, W, H, val[0], val[1], val[2], win[0], st[0], fit[0], fit[1], fit[2], val[0] / fit[0],
            float(valid.mean())), flush=True)
        del agent, mem
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
