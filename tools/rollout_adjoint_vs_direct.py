"""``rollout(m, x0, controls, dt, step_size=s)`` with gradients — H = 16 control intervals of m = 4 fine steps (dt = 1/8,
s = 1/32, exact in binary) — differentiated three ways:

  adjoint  ``adjoint=True`` in one launch: ``nlbac_*_adj_traj`` over the H * m fine intervals (with parameter gradients:
           per chunk of control intervals, + one weight-gradient launch each), nothing kept but ``out``;
  adj c=1  (parameter gradients only) the same with ``adjoint_chunk=1``: one launch and one weight-gradient batch per
           control interval — the kept rows of one interval instead of the largest chunk the batch limit admits;
  chained  the same call with ``rollout.ONE_LAUNCH = False``: one ``nlbac_*_adj_step`` launch per fine step;
  direct   ``adjoint=False``: the one ``*_hold_bwd`` launch on what the forward kept of every fine stage.

One process, alternating rounds, timed with device events after warm-up; a time is forward + backward of one solve.
``--kind unicycle``: the control-affine Unicycle NODE (f_net 5 / g_net 4 layers of 100); ``cars``: the single-net
``NeuralODEModel(12, 10)`` of SimulatedCars.  rows x method x {gradients w.r.t. x0 and the controls, + parameter
gradients}.  Before a row is timed the paths' results are compared: the two adjoint paths' states and input gradients bit
for bit, their parameter gradients within 1e-5 (norm, per tensor), the direct path's states within 1e-5 (its forward
sums f_net's output layer differently when it keeps mask words); the adjoint's input gradients
against the direct ones are reported (``d_in``: largest difference relative to the largest entry — the two agree to
solver accuracy, and at rows on a ReLU kink not even that), not asserted.

    python tools/rollout_adjoint_vs_direct.py [--kind unicycle|cars|both] [--rounds 5] [--reps 3] [--out FILE]

Columns: median over the rounds of the mean time of ``reps`` solves (us), the ratios adjoint / direct and chained /
adjoint, ``torch.cuda.max_memory_allocated`` over one solve per path (MiB, above what was allocated before it), the
chunk (control intervals per backward launch) the adjoint chose, ``d_in``, and time and peak of ``adj c=1``.  Where the direct path's weight-gradient
launch refuses the one batch of H * m * stages * rows rows (2^29 elements per layer), its columns say so.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlbac_amd  # noqa: E402,F401
from nlbac_amd import _lib  # noqa: E402
from nlbac_amd import ode_traj as T  # noqa: E402
from nlbac_amd import rollout as R  # noqa: E402
from nlbac_amd.ode_grid import _sub_grid  # noqa: E402
from nlbac_amd.sac_cbf_clf.model import NeuralODEModel  # noqa: E402

H, DT, S = 16, 1 / 8, 1 / 32
PATHS = ("adjoint", "chained", "direct")
CHUNK1 = "adj c=1"


def run(path, m, x0, c, method, w):
    x, u = x0.detach().requires_grad_(), c.detach().requires_grad_()
    for p in m.parameters():
        p.grad = None
    R.ONE_LAUNCH = path != "chained"
    try:
        out = R.rollout(m, x, u, DT, method=method, step_size=S, adjoint=path != "direct",
                        adjoint_chunk=1 if path == CHUNK1 else None)
        (out * w).sum().backward()
    finally:
        R.ONE_LAUNCH = True
    return out.detach(), x.grad, u.grad, [p.grad for p in m.parameters() if p.grad is not None]


def peak_mib(path, m, x0, c, method, w):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run(path, m, x0, c, method, w)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def check(res):
    o1, gx1, gu1, p1 = res["adjoint"]
    o0, gx0, gu0, p0 = res["chained"]
    assert torch.equal(o1, o0), "chained: states differ"
    assert torch.equal(gx1, gx0) and torch.equal(gu1, gu0), "chained: input gradients differ"
    assert len(p1) == len(p0)
    for a, b in zip(p1, p0):
        assert float((a - b).norm()) <= 1e-5 * max(1e-12, float(b.norm())), "chained: parameter gradients differ"
    if CHUNK1 in res:
        o2, gx2, gu2, p2 = res[CHUNK1]
        assert torch.equal(o1, o2) and torch.equal(gx1, gx2) and torch.equal(gu1, gu2), "chunk 1: states / input gradients differ"
        for a, b in zip(p2, p1):
            assert float((a - b).norm()) <= 1e-5 * max(1e-12, float(b.norm())), "chunk 1: parameter gradients differ"
    if "direct" not in res:
        return float("nan")
    od, gxd, gud, _ = res["direct"]
    rel = lambda a, b: float((a - b).abs().max()) / max(1e-12, float(b.abs().max()))
    # (the direct forward sums f_net's output layer in two parts when it keeps mask words only — see ``rollout`` — so its
    #  states are the adjoint path's to rounding: 64 fine steps of float32 sums)
    assert rel(o1, od) <= 1e-5, "direct: states differ by %.3g" % rel(o1, od)
    return max(rel(gx1, gxd), rel(gu1, gud))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("unicycle", "cars", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--methods", nargs="*", default=["euler", "rk4"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rollout_adjoint_vs_direct.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    assert len(_sub_grid(torch.tensor([0.0, DT]), S)[1]) == 4
    chunks = []
    real_pick = T.AdjointPlan.pick_chunk
    T.AdjointPlan.pick_chunk = lambda self, *args: (chunks.append(real_pick(self, *args)), chunks[-1])[1]
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    emit("rollout(step_size) with gradients: H = %d, m = 4, dt = 1/8, s = 1/32; us per forward + backward; %s" % (
        H, torch.cuda.get_device_name()))
    emit("%-8s %-6s %6s %-7s | %10s %10s %10s | %7s %7s | %9s %9s %9s | %5s %8s | %10s %9s" % (
        "kind", "method", "rows", "grads", "adjoint us", "chained us", "direct us", "adj/dir", "chn/adj", "adj MiB", "chn MiB",
        "dir MiB", "chunk", "d_in", "adj c=1 us", "c=1 MiB"))
    for kind in (("unicycle", "cars") if a.kind == "both" else (a.kind,)):
        torch.manual_seed(0)
        m = NeuralODEModel(3, 3, 6) if kind == "unicycle" else NeuralODEModel(12, 10)
        ns, nc = m.n_s, (m.n_u if m.affine else m.n_carry)
        for method in a.methods:
            for B in a.rows:
                g = torch.Generator(device="cuda").manual_seed(1)
                x0 = torch.rand(B, ns, device="cuda", generator=g) * 2 - 1
                c = torch.rand(H, B, nc, device="cuda", generator=g) * 2 - 1
                w = torch.randn(H + 1, B, ns, device="cuda", generator=g)
                for mode in ("inputs", "params"):
                    for p in m.parameters():
                        p.requires_grad_(mode == "params")
                        p.grad = None
                    paths, refused = list(PATHS) + ([CHUNK1] if mode == "params" else []), None
                    try:
                        run("direct", m, x0, c, method, w)
                    except _lib.NlbacError as e:
                        paths.remove("direct")
                        refused = str(e).split(": ")[-1]
                    res, peak = {}, {}
                    for path in paths:                  # warm-up, agreement, peak memory of one solve
                        run(path, m, x0, c, method, w)
                        peak[path] = peak_mib(path, m, x0, c, method, w)
                        del chunks[:]
                        res[path] = run(path, m, x0, c, method, w)
                        torch.cuda.synchronize()
                        if path == "adjoint":
                            chunk = chunks[-1]
                    d_in = check(res)
                    res.clear()
                    tm = {p: [] for p in paths}
                    for _ in range(a.rounds):
                        for path in paths:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(a.reps):
                                run(path, m, x0, c, method, w)
                            e1.record()
                            e1.synchronize()
                            tm[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                    med = {p: statistics.median(v) for p, v in tm.items()}
                    c1 = " | %10.1f %9.1f" % (med[CHUNK1], peak[CHUNK1]) if CHUNK1 in med else " | %10s %9s" % ("-", "-")
                    if refused is None:
                        emit("%-8s %-6s %6d %-7s | %10.1f %10.1f %10.1f | %7.2f %7.2f | %9.1f %9.1f %9.1f | %5d %8.1e" % (
                            kind, method, B, mode, med["adjoint"], med["chained"], med["direct"], med["adjoint"] / med["direct"],
                            med["chained"] / med["adjoint"], peak["adjoint"], peak["chained"], peak["direct"], chunk, d_in) + c1)
                    else:
                        emit("%-8s %-6s %6d %-7s | %10.1f %10.1f %10s | %7s %7.2f | %9.1f %9.1f %9s | %5d %8s%s   direct: %s" % (
                            kind, method, B, mode, med["adjoint"], med["chained"], "refused", "-", med["chained"] / med["adjoint"],
                            peak["adjoint"], peak["chained"], "-", chunk, "-", c1, refused))


if __name__ == "__main__":
    main()
