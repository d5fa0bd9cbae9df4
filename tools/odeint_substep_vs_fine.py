"""``odeint_grid(m, y0, t, step_size=s)`` — T = 5 output points over N = 16 and N = 64 fine steps — against the way the
same result was had before ``step_size``: ``odeint_grid`` on the fine grid itself (N + 1 points, every fine state
materialised, and with a backward every fine state's gradient) followed by the linear interpolation as torch ops.  One
process, alternating rounds, timed with device events after warm-up.  ``--kind unicycle``: the control-affine Unicycle
NODE (f_net 5 / g_net 4 layers of 100); ``cars``: the single-net ``NeuralODEModel(12, 10)`` of SimulatedCars.
rows x method x N x {forward only, + gradient w.r.t. y0, + parameter gradients}.  Before a time is printed the two
paths' outputs are compared (bitwise at fine-grid points, within 4 * 2^-24 (|a0| + |a1|) of the float64 interpolation
elsewhere) and their gradients (1e-5 of the baseline's largest entry per tensor).

    python tools/odeint_substep_vs_fine.py [--kind unicycle|cars|both] [--rounds 7] [--reps 5]

Columns: median over the rounds of the mean time of ``reps`` solves (us), the ratio fine / sub, library calls per solve,
the peak of torch's allocator over one solve (MiB, above what was allocated before it) and the sub-stepped path's spread
(max - min over the rounds).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib  # noqa: E402
from nlbac_amd.ode_grid import _sub_grid, odeint_grid  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

# T = 5 output points, the interior ones between fine-grid points; the span and the step sizes are exact in binary
GRID = [0.0, 0.03, 0.06, 0.1, 0.125]
STEPS = {16: 1 / 128, 64: 1 / 512}


FINE = [None]


def interpolate(fine, where, theta):
    pts = [fine[0]]
    for j in range(1, len(GRID)):
        a0, a1, th = fine[where[j]], fine[where[j] + 1], theta[j - 1]
        pts.append(a1 if th == 1.0 else (a0 if th == 0.0 else a0 + th * (a1 - a0)))
    return torch.stack(pts)


def run(path, m, y0, method, mode, w, sub):
    s, taus, where, theta = sub
    def fine_solve(y):
        fine = odeint_grid(m, y, taus, method=method)
        FINE[0] = fine.detach()       # (the fine states of THIS keep-mode: their last bits depend on it, see rollout)
        return interpolate(fine, where, theta)

    solve = (lambda y: odeint_grid(m, y, GRID, method=method, step_size=s)) if path == "sub" else fine_solve
    if mode == "fwd":
        with torch.no_grad():
            return solve(y0), None, []
    y = y0.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    out = solve(y)
    (out * w).sum().backward()
    return out.detach(), y.grad, [p.grad for p in m.parameters() if p.grad is not None]


def check(res, m, sub):
    s, taus, where, theta = sub
    (o1, g1, p1), (o0, g0, p0) = res["sub"], res["fine"]
    ns, fine = m.n_s, FINE[0]
    for j in range(len(GRID)):
        if j == 0 or theta[j - 1] in (0.0, 1.0):
            assert torch.equal(o1[j], o0[j]), "output %d differs" % j
            continue
        a0, a1 = fine[where[j]][:, :ns].double(), fine[where[j] + 1][:, :ns].double()
        err = (o1[j][:, :ns].double() - (a0 + theta[j - 1] * (a1 - a0))).abs()
        assert bool((err <= 4 * 2.0 ** -24 * (a0.abs() + a1.abs())).all()), "output %d is off the interpolation" % j
    for a, b in zip([g1] + list(p1), [g0] + list(p0)):
        if a is not None:
            assert float((a - b).abs().max()) <= 1e-5 * max(1e-30, float(b.abs().max())), "gradients differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--methods", nargs="*", default=["euler", "rk4"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    calls = []
    real = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    subs = {}
    for N, s in STEPS.items():
        taus, hs, ofs, theta = _sub_grid(GRID, s)
        assert len(hs) == N
        where = {j: i for i in range(N) for j in range(ofs[i], ofs[i + 1])}
        subs[N] = (s, torch.tensor(taus, dtype=torch.float64), where, theta)
    print("%-8s %-6s %6s %3s %-7s | %10s %10s | %8s | %5s %6s | %9s %9s | %8s" % (
        "kind", "method", "rows", "N", "mode", "sub us", "fine us", "fine/sub", "l_sub", "l_fine", "MiB sub", "MiB fine", "sp_sub"))
    paths = ("sub", "fine")
    for kind in (("unicycle", "cars") if a.kind == "both" else (a.kind,)):
        torch.manual_seed(0)
        m = NeuralODEModel(3, 3, 6) if kind == "unicycle" else NeuralODEModel(12, 10)
        width = m.n_s + (m.n_u if m.affine else m.n_carry)
        for method in a.methods:
            for B in a.rows:
                g = torch.Generator(device="cuda").manual_seed(1)
                y0 = torch.rand(B, width, device="cuda", generator=g) * 2 - 1
                w = torch.randn(len(GRID), B, width, device="cuda", generator=g)
                for N in STEPS:
                    for mode in ("fwd", "inputs", "params"):
                        for p in m.parameters():
                            p.requires_grad_(mode == "params")
                            p.grad = None
                        res, launches, peak = {}, {}, {}
                        try:      # (the weight-gradient launch takes fewer than 2^29 / width rows: N * stages * rows here)
                            for path in paths:
                                run(path, m, y0, method, mode, w, subs[N])
                        except _lib.NlbacError as e:
                            print("%-8s %-6s %6d %3d %-7s | both paths refused: %s" % (kind, method, B, N, mode, str(e).split(": ")[-1]),
                                  flush=True)
                            continue
                        for path in paths:                  # warm-up, agreement, library calls and peak memory per solve
                            run(path, m, y0, method, mode, w, subs[N])
                            torch.cuda.synchronize()
                            del calls[:]
                            res[path] = None
                            torch.cuda.reset_peak_memory_stats()
                            before = torch.cuda.memory_allocated()
                            res[path] = run(path, m, y0, method, mode, w, subs[N])
                            torch.cuda.synchronize()
                            peak[path] = (torch.cuda.max_memory_allocated() - before) / 2.0 ** 20
                            launches[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                        check(res, m, subs[N])
                        res.clear()
                        FINE[0] = None
                        tm = {p: [] for p in paths}
                        for _ in range(a.rounds):
                            for path in paths:
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _ in range(a.reps):
                                    run(path, m, y0, method, mode, w, subs[N])
                                e1.record()
                                e1.synchronize()
                                tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                        med = {p: statistics.median(v) for p, v in tm.items()}
                        print("%-8s %-6s %6d %3d %-7s | %10.1f %10.1f | %8.3f | %5d %6d | %9.1f %9.1f | %8.1f" % (
                            kind, method, B, N, mode, med["sub"], med["fine"], med["fine"] / med["sub"], launches["sub"],
                            launches["fine"], peak["sub"], peak["fine"], max(tm["sub"]) - min(tm["sub"])), flush=True)


if __name__ == "__main__":
    main()
