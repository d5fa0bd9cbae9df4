"""``nlbac_amd.ode_dense.odeint_dense`` on a 17-point grid over [0, 0.32] against what a user had before it and against
its floor — forward only, + backward with input gradients, + parameter gradients — on 8192 rows, in one process,
alternating rounds, timed with device events after warm-up:

  dense    ``odeint_dense(m, y0, t)``: ONE adaptive dopri5 solve read at the 16 output points;
  restart  the chain of 16 dopri5 solves restarted at every grid point — the other solution (initial-step selection at
           every point, steps cut at the grid).  Forward only it is 16 ``odeint(..., method="dopri5")`` calls; with a
           backward it is ``rollout(..., method="dopri5")`` with the carried columns as every interval's control, which IS
           that chain as one autograd node (``odeint``'s own solver keeps one solve's state, so a chain of its calls
           cannot be differentiated as a whole);
  floor    one ``odeint`` over [0, 0.32]: the same solve without interior points.  dense - floor is what the two new
           kernels and the carry launches cost (the floor's chain carries the gradients inside its backward launches).
           With input gradients only, ``odeint``'s solver still keeps activation rows where the other two keep ReLU mask
           words: compare dense and floor under "+d/dth", where all three keep rows.

``--kind unicycle``: the control-affine Unicycle NODE at the reference width (f_net 5 / g_net 4 layers of 100);
``cars``: the single-net ``NeuralODEModel(12, 10)`` of SimulatedCars.

    python tools/odeint_dense_probe.py [--kind unicycle|cars|both] [--rows 8192] [--rounds 7] [--reps 5]

Columns: median over the rounds of the mean time of ``reps`` calls (us), restart / dense, dense - floor, the library
calls per call of each path, the steps each accepted (restart: summed over its 16 solves), and dense's spread (max - min
over the rounds)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib, ode_dense  # noqa: E402
from nlbac_amd.odeint import odeint  # noqa: E402
from nlbac_amd.rollout import rollout  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

T, T_END = 17, 0.32
PATHS = ("dense", "restart", "floor")


def run(path, m, y0, t, mode, w):
    """One call of ``path``; returns (out, d/dy0 or None, accepted steps)."""
    ns = m.n_s
    steps_of = lambda sv: len(sv.ctx["steps"])
    if mode == "none":
        with torch.no_grad():
            if path == "dense":
                return ode_dense.odeint_dense(m, y0, t), None, steps_of(ode_dense.solver_of(m, "none"))
            if path == "floor":
                return odeint(m, y0, t[[0, -1]], method="dopri5"), None, steps_of(m._odeint_solver)
            ys, steps = [y0], 0
            for k in range(T - 1):
                ys.append(odeint(m, ys[-1], t[k:k + 2], method="dopri5")[-1])
                steps += steps_of(m._odeint_solver)
            return torch.stack(ys), None, steps
    y = y0.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    if path == "dense":
        out = ode_dense.odeint_dense(m, y, t)
        (out * w).sum().backward()
        steps = steps_of(ode_dense.solver_of(m, mode))
    elif path == "floor":
        out = odeint(m, y, t[[0, -1]], method="dopri5")
        (out * w[[0, -1]]).sum().backward()
        steps = steps_of(m._odeint_solver)
    else:
        out = rollout(m, y[:, :ns], y[:, ns:].unsqueeze(0).expand(T - 1, -1, -1).contiguous(), T_END / (T - 1), method="dopri5")
        (out * w[:, :, :ns]).sum().backward()
        steps = sum(steps_of(sv) for sv in m.__dict__["_rollout_solvers"][mode][:T - 1])
    return out, y.grad, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    calls = []
    real = _lib.call
    _lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    t = torch.linspace(0.0, T_END, T)
    print("%-8s %6s %-7s | %10s %10s %10s | %9s %11s | %7s %9s %7s | %6s %8s %6s | %8s" % (
        "kind", "rows", "mode", "dense us", "restart us", "floor us", "restart/1", "dense-floor", "l_dense", "l_restart",
        "l_floor", "s_dens", "s_restrt", "s_flor", "sp_dense"))
    for kind in (("unicycle", "cars") if a.kind == "both" else (a.kind,)):
        torch.manual_seed(0)
        m = NeuralODEModel(3, 3, 6) if kind == "unicycle" else NeuralODEModel(12, 10)
        width = m.n_s + (m.n_u if m.affine else m.n_carry)
        g = torch.Generator(device="cuda").manual_seed(1)
        y0 = torch.rand(a.rows, width, device="cuda", generator=g) * 2 - 1
        w = torch.randn(T, a.rows, width, device="cuda", generator=g)
        for mode in ("none", "inputs", "params"):      # what is kept: nothing, ReLU mask words, activation rows
            for p in m.parameters():
                p.requires_grad_(mode == "params")
            res, launches, steps = {}, {}, {}
            for path in PATHS:                              # warm-up, library calls and accepted steps per call
                run(path, m, y0, t, mode, w)
                torch.cuda.synchronize()
                del calls[:]
                res[path] = run(path, m, y0, t, mode, w)
                torch.cuda.synchronize()
                launches[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                steps[path] = res[path][2]
            # the dense solve IS the floor's solve: its last point carries the floor's bits (not under "inputs", where
            # odeint's solver still keeps rows and the two run different forward kernels: see rollout on mask words)
            if mode != "inputs":
                assert torch.equal(res["dense"][0][-1], res["floor"][0][-1]), "dense / one odeint: the last point differs"
            tm = {p: [] for p in PATHS}
            for _ in range(a.rounds):
                for path in PATHS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        run(path, m, y0, t, mode, w)
                    e1.record()
                    e1.synchronize()
                    tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            med = {p: statistics.median(v) for p, v in tm.items()}
            print("%-8s %6d %-7s | %10.1f %10.1f %10.1f | %9.3f %11.1f | %7d %9d %7d | %6d %8d %6d | %8.1f" % (
                kind, a.rows, {"none": "fwd", "inputs": "+d/dy0", "params": "+d/dth"}[mode], med["dense"], med["restart"], med["floor"],
                med["restart"] / med["dense"], med["dense"] - med["floor"], launches["dense"], launches["restart"],
                launches["floor"], steps["dense"], steps["restart"], steps["floor"],
                max(tm["dense"]) - min(tm["dense"])), flush=True)


if __name__ == "__main__":
    main()
