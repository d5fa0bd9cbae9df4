"""Time of one NODE fit on trajectory windows (``SAC_CBF_CLF.fit_node_windows``, H in {2, 3, 5}) beside the same build's
one-step fit (``fit_node_rows``) at nb rows, and of the window gather + trajectory loss launches on their own.

    python tools/fit_windows_probe.py [--rows 32768] [--rounds 7] [--reps 5]

Unicycle (euler, rk4) and SimulatedCars (rk4).  The replay holds synthetic episodes of 200 steps (chained observations,
so most windows are valid); every fit includes its Adam step; times are medians over the rounds of the mean of ``reps``
calls between two device events, after a warm-up.  ``gather`` is one ``sample_windows`` call with the start rows already
on the device (one ``nlbac_gather_windows`` launch; the host draw of nb indices is the caller's cost as in
``sample_rows``), ``loss`` is ``nlbac_traj_mse_fwd_bwd`` + ``nlbac_sum_partials``.  The one-step column is
``fit_node_rows`` — the path the window fit leaves untouched — measured in the same process on the same agent.  No bar
hangs on these numbers; the comparison a reader will want is H x the one-step fit, and ``x1step`` = fit / (H x 1-step)
is printed beside each window fit.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import synth  # noqa: E402
from nlbac_amd.node_fit import loss_blocks, traj_mse_launch  # noqa: E402
from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory  # noqa: E402
from nlbac_amd.sac_cbf_clf.sac_cbf_clf import SAC_CBF_CLF  # noqa: E402
from oracle.nlbac_oracle import Args  # noqa: E402

HORIZONS = (2, 3, 5)
EPISODE = 200


def make_agent(env_name, solver):
    env = synth.fixture_env(env_name, 0)
    agent = SAC_CBF_CLF(env.obs_dim, env.action_space, env, Args(batch_size=256, hidden_size=256, seed=0, cuda=True))
    agent.solver = solver
    return agent, env


def fill(agent, env_name, env, n):
    """n replay rows: synthetic transitions whose next observation is copied into the next row's observation, in
    episodes of EPISODE steps."""
    tr = synth.transitions(env_name, n, seed=1, env=env)
    rows = agent._rows_from_host(tuple(tr[f] for f in synth.fields(env_name)))
    lay = agent.lay
    inside = (np.arange(n - 1) + 1) % EPISODE != 0
    idx = torch.from_numpy(np.nonzero(inside)[0])
    rows[idx + 1, lay.obs:lay.obs + lay.obs_dim] = rows[idx, lay.nobs:lay.nobs + lay.obs_dim]
    mem = DeviceReplayMemory(n, 0, agent)
    mem.push_rows(rows)
    return mem


def timed(fn, rounds, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(ts), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    nb = a.rows
    print("%-14s %-6s %6s %2s | %10s %8s | %10s %8s | %9s %9s | %6s" % (
        "env", "solver", "rows", "H", "fit us", "spread", "1-step us", "x1step", "gather us", "loss us", "valid"))
    for env_name, solver in (("Unicycle", "euler"), ("Unicycle", "rk4"), ("SimulatedCars", "rk4")):
        agent, env = make_agent(env_name, solver)
        mem = fill(agent, env_name, env, nb)
        one_rows = mem.sample_rows(nb)
        one, _ = timed(lambda: agent.fit_node_rows(one_rows), a.rounds, a.reps)
        ns = agent.task.n_s
        for H in HORIZONS:
            starts = torch.randperm(nb, device="cuda", generator=torch.Generator(device="cuda").manual_seed(H))
            rows, valid = mem.sample_windows(nb, H, idx=starts)
            counts = mem.window_counts
            fit, spread = timed(lambda: agent.fit_node_windows(rows, valid, counts), a.rounds, a.reps)
            gather, _ = timed(lambda: mem.sample_windows(nb, H, out=rows, idx=starts), a.rounds, a.reps)
            w = agent._fit_windows_ws(nb, H)
            scratch = torch.empty(1, device="cuda")
            assert w["part"].numel() == loss_blocks(H, nb, ns)
            loss, _ = timed(lambda: traj_mse_launch(w["xs"], w["target"], valid, counts, H, nb, ns, w["dout"][1:],
                                                    w["part"], scratch.data_ptr()), a.rounds, a.reps)
            print("%-14s %-6s %6d %2d | %10.1f %8.1f | %10.1f %8.2f | %9.1f %9.1f | %6.3f" % (
                env_name, solver, nb, H, fit, spread, one, fit / (H * one), gather, loss, float(valid.mean())), flush=True)
        del agent, mem
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
