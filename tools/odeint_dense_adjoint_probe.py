"""``nlbac_amd.ode_dense.odeint_dense_adjoint`` on a 17-point grid over [0, 0.32] against the two ways a user had to the same
gradients — forward + backward with input gradients, + parameter gradients — on 8192 rows, in one process, alternating
rounds, timed with device events after warm-up:

  adjoint  ``odeint_dense_adjoint(m, y0, t)``: ONE dense dopri5 solve, the continuous adjoint walked over the 16 intervals;
  direct   ``odeint_dense(m, y0, t)``: the same solve, back-propagation through the accepted steps (activation and dz rows
           of every accepted step are kept);
  restart  the chain of 16 ``odeint_adjoint`` solves restarted at every grid point — ``rollout(..., method="dopri5",
           adjoint=True)`` with the carried columns as every interval's control, which IS that chain as one autograd node
           (another forward solution: the initial-step selection runs at every point and steps are cut there).

``--kind unicycle``: the control-affine Unicycle NODE at the reference width (f_net 5 / g_net 4 layers of 100);
``cars``: the single-net ``NeuralODEModel(12, 10)`` of SimulatedCars.  Every path runs on a model of its own (the same
weights), so that what a path allocates — slot pools and scratch included — is its own.

    python tools/odeint_dense_adjoint_probe.py [--kind unicycle|cars|both] [--rows 8192] [--rounds 7] [--reps 3] [--t-end 0.32]

Columns, per path: median over the rounds of the mean time of ``reps`` forward + backward calls (us) and its spread (max -
min over the rounds); the peak of
``torch.cuda.max_memory_allocated`` over a path's first two calls above what was allocated before them (MiB: pools,
scratch and kept buffers); library calls, host waits on the control block and the host time spent in them (us) per call;
accepted forward steps and (adjoint) the attempts of the 16 adjoint solves.  ``us/iv``: adjoint minus a forward-only
dense solve, per interval."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib, ode_dense  # noqa: E402
from nlbac_amd.ode_ctl import ControlBlockReader  # noqa: E402
from nlbac_amd.rollout import rollout  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

T, T_END = 17, 0.32
PATHS = ("adjoint", "direct", "restart")


def run(path, m, y0, t, w):
    """One forward + backward of ``path``; returns (d/dy0, accepted forward steps, attempts of the adjoint solves)."""
    ns = m.n_s
    y = y0.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    if path == "adjoint":
        out = ode_dense.odeint_dense_adjoint(m, y, t)
        (out * w).sum().backward()
        sv = ode_dense.solver_of(m, ode_dense.ADJOINT)
        return y.grad, len(sv.ctx["steps"]), sum(e[0][0][2] for e in sv.ctx["adjoint_info"])
    if path == "direct":
        out = ode_dense.odeint_dense(m, y, t)
        (out * w).sum().backward()
        mode = "params" if any(p.requires_grad for p in m.parameters()) else "inputs"
        return y.grad, len(ode_dense.solver_of(m, mode).ctx["steps"]), 0
    out = rollout(m, y[:, :ns], y[:, ns:].unsqueeze(0).expand(T - 1, -1, -1).contiguous(), T_END / (T - 1), method="dopri5",
                  adjoint=True)
    (out * w[:, :, :ns]).sum().backward()
    return y.grad, 0, 0


def forward_only(m, y0, t):
    with torch.no_grad():
        ode_dense.odeint_dense_adjoint(m, y0, t)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    global T_END
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--t-end", type=float, default=T_END, help="the grid's span (more accepted steps on a longer one)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    T_END = a.t_end
    calls, waits = [], []
    real_call, real_read = _lib.call, ControlBlockReader.read
    _lib.call = lambda name, *args: (calls.append(name), real_call(name, *args))[1]

    def read(self, ctx, P, before_wait=None):
        t0 = time.perf_counter()
        c = real_read(self, ctx, P, before_wait)
        if c is not None:
            waits.append(time.perf_counter() - t0)
        return c
    ControlBlockReader.read = read
    t = torch.linspace(0.0, T_END, T)
    print("%-8s %6s %-7s %-8s | %10s %8s %9s | %6s %6s %9s | %6s %8s | %8s" % (
        "kind", "rows", "mode", "path", "fwd+bwd us", "spread", "peak MiB", "calls", "waits", "wait us", "steps", "attempts",
        "us/iv"))
    for kind in (("unicycle", "cars") if a.kind == "both" else (a.kind,)):
        g = torch.Generator(device="cuda").manual_seed(1)
        width = 5 if kind == "unicycle" else 12
        y0 = torch.rand(a.rows, width, device="cuda", generator=g) * 2 - 1
        w = torch.randn(T, a.rows, width, device="cuda", generator=g) / a.rows
        for mode in ("inputs", "params"):
            models, peak, info, n_calls, n_waits, wait_us = {}, {}, {}, {}, {}, {}
            for path in PATHS:
                torch.manual_seed(0)
                m = models[path] = NeuralODEModel(3, 3, 6) if kind == "unicycle" else NeuralODEModel(12, 10)
                for p in m.parameters():
                    p.requires_grad_(mode == "params")
                m.device_handles()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                run(path, m, y0, t, w)              # (the first call sizes the pools; the second runs in them)
                run(path, m, y0, t, w)
                torch.cuda.synchronize()
                peak[path] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                del calls[:], waits[:]
                info[path] = run(path, m, y0, t, w)
                torch.cuda.synchronize()
                n_calls[path] = sum(1 for n in calls if n.startswith("nlbac_"))
                n_waits[path], wait_us[path] = len(waits), sum(waits) * 1e6
            # the adjoint against the direct gradient of the same solve: solver tolerance
            ga, gd = info["adjoint"][0], info["direct"][0]
            dist = float((ga - gd).norm() / gd.norm())
            forward_only(models["adjoint"], y0, t)
            tm, tf = {p: [] for p in PATHS}, []
            for _ in range(a.rounds):
                for path in PATHS:
                    tm[path].append(timed(lambda: run(path, models[path], y0, t, w), a.reps))
                tf.append(timed(lambda: forward_only(models["adjoint"], y0, t), a.reps))
            med = {p: statistics.median(v) for p, v in tm.items()}
            for path in PATHS:
                per_iv = "%8.1f" % ((med[path] - statistics.median(tf)) / (T - 1)) if path == "adjoint" else "%8s" % "-"
                print("%-8s %6d %-7s %-8s | %10.1f %8.1f %9.1f | %6d %6d %9.1f | %6d %8d | %s" % (
                    kind, a.rows, {"inputs": "+d/dy0", "params": "+d/dth"}[mode], path, med[path],
                    max(tm[path]) - min(tm[path]), peak[path],
                    n_calls[path], n_waits[path], wait_us[path], info[path][1], info[path][2], per_iv), flush=True)
            print("%-8s %6d %-7s adjoint vs direct d/dy0: rel L2 %.3g; memory direct / adjoint %.1f, restart / adjoint %.1f; "
                  "forward only %.1f us" % (kind, a.rows, {"inputs": "+d/dy0", "params": "+d/dth"}[mode], dist,
                                            peak["direct"] / peak["adjoint"], peak["restart"] / peak["adjoint"],
                                            statistics.median(tf)), flush=True)
            del models


if __name__ == "__main__":
    main()
