"""One-launch trajectory kernels against the chained one-interval solves (``nlbac_amd.rollout.ONE_LAUNCH`` on / off),
in one process, alternating rounds, timed with device events.  ``--kind unicycle`` (default): the control-affine
Unicycle NODE (f_net 5 / g_net 4 layers of 100); ``cars``: the single-net ``NeuralODEModel(12, 10)`` of SimulatedCars;
``quadrotor``: the normalised 8 -> 6 single-net NODE.  rows x H x method x {forward only, forward + backward w.r.t.
x0 / controls, + parameter gradients}.  The two paths' outputs are asserted equal before a time is printed; the
single-net kinds also print each path's round-to-round spread (max - min over the rounds).

    python tools/microbench_rollout.py [--kind unicycle|cars|quadrotor] [--rounds 5] [--reps 10]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib  # noqa: E402
from nlbac_amd import rollout as R  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

PEAK = 157.3e12                      # fp32 MFMA peak of the MI355X


def run(m, x0, c, method, mode, w):
    if mode == "fwd":
        with torch.no_grad():
            return R.rollout(m, x0, c, 0.02, method=method), None
    x = x0.detach().requires_grad_()
    u = c.detach().requires_grad_()
    out = R.rollout(m, x, u, 0.02, method=method)
    (out * w).sum().backward()
    return out, (x.grad, u.grad)


def build(kind):
    """The model of a kind, its state / control widths."""
    if kind == "unicycle":
        return NeuralODEModel(3, 3, 6), 3, 2
    if kind == "cars":
        return NeuralODEModel(12, 10), 10, 2
    g = torch.Generator().manual_seed(2)
    r = lambda n, lo, hi: torch.rand(n, generator=g) * (hi - lo) + lo
    norm = (r(8, -0.5, 0.5), r(8, 0.5, 2.0), r(6, -0.5, 0.5), r(6, 0.5, 2.0))
    return NeuralODEModel(8, 6, normalizer=tuple(v.numpy() for v in norm)), 6, 2


def flop_per_row_stage(m):
    """2 x MACs of the field's nets per row and stage, from their layer sizes."""
    return 2 * sum(l.in_features * l.out_features for l in m.modules() if isinstance(l, torch.nn.Linear))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "quadrotor"), default="unicycle")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    m, ns, nc = build(a.kind)
    flop = flop_per_row_stage(m)
    spread = a.kind != "unicycle"
    calls = []
    real = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    print("%-6s %6s %3s %-7s | %10s %10s %7s | %7s %7s | %9s %6s" % (
        "method", "rows", "H", "mode", "one us", "chain us", "ratio", "l_one", "l_chain", "fwd TF/s", "%peak")
          + (" | %8s %8s" % ("sp_one", "sp_chain") if spread else ""))
    for method in ("euler", "rk4"):
        S = 1 if method == "euler" else 4
        for B in (8192, 32768):
            for H in (1, 4, 16):
                g = torch.Generator(device="cuda").manual_seed(1)
                x0 = torch.rand(B, ns, device="cuda", generator=g) * 2 - 1
                c = torch.rand(H, B, nc, device="cuda", generator=g) * 2 - 1
                w = torch.randn(H + 1, B, ns, device="cuda", generator=g)
                for mode in ("fwd", "inputs", "params"):
                    for p in m.parameters():
                        p.requires_grad_(mode == "params")
                        p.grad = None
                    res, launches = {}, {}
                    for on in (True, False):                 # warm-up, equality, launches per rollout
                        R.ONE_LAUNCH = on
                        run(m, x0, c, method, mode, w)
                        torch.cuda.synchronize()
                        del calls[:]
                        res[on] = run(m, x0, c, method, mode, w)
                        torch.cuda.synchronize()
                        launches[on] = sum(1 for n in calls if n.startswith("nlbac_"))
                    assert torch.equal(res[True][0], res[False][0]), "outputs differ"
                    if res[True][1] is not None:
                        assert all(torch.equal(p, q) for p, q in zip(res[True][1], res[False][1])), "input grads differ"
                    t = {True: [], False: []}
                    for _ in range(a.rounds):
                        for on in (True, False):
                            R.ONE_LAUNCH = on
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(a.reps):
                                run(m, x0, c, method, mode, w)
                            e1.record()
                            e1.synchronize()
                            t[on].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                    one, chain = min(t[True]), min(t[False])
                    tf = flop * B * S * H / (one * 1e-6) if mode == "fwd" else float("nan")
                    print("%-6s %6d %3d %-7s | %10.1f %10.1f %7.3f | %7d %7d | %9.1f %6.1f" % (
                        method, B, H, mode, one, chain, chain / one, launches[True], launches[False], tf / 1e12,
                        100 * tf / PEAK)
                          + (" | %8.1f %8.1f" % (max(t[True]) - one, max(t[False]) - chain) if spread else ""), flush=True)
    R.ONE_LAUNCH = True


if __name__ == "__main__":
    main()
