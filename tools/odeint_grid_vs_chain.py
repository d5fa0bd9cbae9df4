"""``nlbac_amd.ode_grid.odeint_grid`` on a 17-point time grid against (a) the chain of 16 ``odeint`` calls on the same
grid — forward only: ``odeint``'s solver keeps one solve's state, so a chain of its calls cannot be differentiated as a
whole — and (b) its own chained path (``nlbac_amd.rollout.ONE_LAUNCH`` off), in one process, alternating rounds, timed
with device events after warm-up.  ``--kind unicycle``: the control-affine
Unicycle NODE (f_net 5 / g_net 4 layers of 100); ``cars``: the single-net ``NeuralODEModel(12, 10)`` of SimulatedCars.
rows x method x {forward only, + gradient w.r.t. y0, + parameter gradients}.  The three paths' outputs are asserted
bit-equal before a time is printed (the one-launch and chained paths' input gradients too).

    python tools/odeint_grid_vs_chain.py [--kind unicycle|cars|both] [--rounds 7] [--reps 5]

Columns: median over the rounds of the mean time of ``reps`` solves (us), the two ratios against the one-launch path,
library calls per solve, and the one-launch path's spread (max - min over the rounds).
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
from nlbac_amd.ode_grid import odeint_grid  # noqa: E402
from nlbac_amd.odeint import odeint  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

T = 17
# a non-uniform grid: the intervals cycle through 0.02, 0.03, 0.005, 0.045
GRID = [0.0]
for _k in range(T - 1):
    GRID.append(GRID[-1] + (0.02, 0.03, 0.005, 0.045)[_k % 4])


def chain_of_odeint(m, y0, t, method):
    ys = [y0]
    for k in range(len(t) - 1):
        ys.append(odeint(m, ys[-1], t[k:k + 2], method=method)[-1])
    return torch.stack(ys)


def run(path, m, y0, t, method, mode, w):
    R.ONE_LAUNCH = path != "chain"
    if mode == "fwd":
        with torch.no_grad():
            return (chain_of_odeint(m, y0, t, method) if path == "odeint" else odeint_grid(m, y0, t, method=method)), None
    y = y0.detach().requires_grad_()
    out = odeint_grid(m, y, t, method=method)
    (out * w).sum().backward()
    return out, y.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[8192, 32768])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    calls = []
    real = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    t = torch.tensor(GRID)
    print("%-8s %-6s %6s %-7s | %10s %10s %10s | %7s %7s | %5s %7s %8s | %8s" % (
        "kind", "method", "rows", "mode", "one us", "chain us", "odeint us", "chain/1", "odeint/1", "l_one", "l_chain",
        "l_odeint", "sp_one"))
    for kind in (("unicycle", "cars") if a.kind == "both" else (a.kind,)):
        torch.manual_seed(0)
        m = NeuralODEModel(3, 3, 6) if kind == "unicycle" else NeuralODEModel(12, 10)
        width = m.n_s + (m.n_u if m.affine else m.n_carry)
        for method in ("euler", "rk4"):
            for B in a.rows:
                g = torch.Generator(device="cuda").manual_seed(1)
                y0 = torch.rand(B, width, device="cuda", generator=g) * 2 - 1
                w = torch.randn(T, B, width, device="cuda", generator=g)
                for mode in ("fwd", "inputs", "params"):
                    paths = ("one", "chain", "odeint") if mode == "fwd" else ("one", "chain")
                    for p in m.parameters():
                        p.requires_grad_(mode == "params")
                        p.grad = None
                    res, launches = {}, {}
                    for path in paths:                      # warm-up, equality, library calls per solve
                        run(path, m, y0, t, method, mode, w)
                        torch.cuda.synchronize()
                        del calls[:]
                        res[path] = run(path, m, y0, t, method, mode, w)
                        torch.cuda.synchronize()
                        launches[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                    assert torch.equal(res["one"][0], res["chain"][0]), "one launch / chained: outputs differ"
                    if mode == "fwd":
                        assert torch.equal(res["one"][0], res["odeint"][0]), "odeint_grid / chain of odeint: outputs differ"
                    else:
                        assert torch.equal(res["one"][1], res["chain"][1]), "one launch / chained: input gradients differ"
                    tm = {p: [] for p in paths}
                    for _ in range(a.rounds):
                        for path in paths:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(a.reps):
                                run(path, m, y0, t, method, mode, w)
                            e1.record()
                            e1.synchronize()
                            tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                    med = {p: statistics.median(v) for p, v in tm.items()}
                    med.setdefault("odeint", float("nan"))
                    print("%-8s %-6s %6d %-7s | %10.1f %10.1f %10.1f | %7.3f %7.3f | %5d %7d %8d | %8.1f" % (
                        kind, method, B, mode, med["one"], med["chain"], med["odeint"], med["chain"] / med["one"],
                        med["odeint"] / med["one"], launches["one"], launches["chain"], launches.get("odeint", 0),
                        max(tm["one"]) - min(tm["one"])), flush=True)
    R.ONE_LAUNCH = True


if __name__ == "__main__":
    main()
