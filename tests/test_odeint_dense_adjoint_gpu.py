"""GPU: ``nlbac_amd.ode_dense.odeint_dense_adjoint`` — ``odeint_dense``'s solve with the continuous adjoint walked over
the grid's intervals as its backward — against ``odeint_adjoint`` where the two must coincide bit for bit (two time
points), against ``odeint_dense`` (the same values; its direct gradient to solver tolerance), against the CPU reference
composed from the oracle's pieces (``dense_adjoint_common``), and against itself (determinism, a solver state of its own,
what a forward holds).  The hand-over kernel ``nlbac_adj_dense_restart`` is also run alone.

Two width-64 NODEs: the Unicycle one on 200 rows (ragged against the 32-row tile) and the single-net SimulatedCars one on
64 rows, five grid points each, two accepted forward steps holding two outputs each."""
import numpy as np
import pytest
import torch

import dense_adjoint_common as A
from common import vec_close
from test_odeint_dense_gpu import node_of

pytestmark = pytest.mark.gpu
TOL = 1e-4


def run(m, y0, t, dout, adjoint_params=None, entry=None):
    """(out, d/dy0, flat d/d theta or None) of ``sum(out * dout)``."""
    from nlbac_amd.ode_dense import odeint_dense_adjoint
    yy = y0.clone().requires_grad_(True)
    if entry is None:
        out = odeint_dense_adjoint(m, yy, t, adjoint_params=adjoint_params)
    else:
        out = entry(m, yy, t)
    ps = list(m.parameters()) if adjoint_params is None else []
    g = torch.autograd.grad((out * dout).sum(), [yy] + ps)
    return out.detach(), g[0], (torch.cat([v.reshape(-1) for v in g[1:]]) if ps else None)


def attempts_of(m):
    """Attempts of every interval's adjoint solve, last interval first (``ctx["adjoint_info"]``: one ``_adj_dopri`` record
    per interval — per problem (step size, error ratio, attempts))."""
    from nlbac_amd import ode_dense
    return [e[0][0][2] for e in ode_dense.solver_of(m, ode_dense.ADJOINT).ctx["adjoint_info"]]


def inputs(name):
    c = A.case(name)
    return c, node_of(name), c["y0"].cuda(), c["t"], c["dout"].cuda()


@pytest.mark.parametrize("name", A.NAMES)
@pytest.mark.parametrize("adjoint_params", [None, ()])
def test_two_points_are_odeint_adjoint_itself(name, adjoint_params):
    """One interval: the same forward values, and carry, restart and finish reduce to ``odeint_adjoint``'s launches — the
    same bits in ``out``, in d/dy0 (state and carried columns, the output gradient nonzero on both points and all
    columns) and in every parameter gradient."""
    from nlbac_amd.odeint import odeint_adjoint
    c, m, y0, t, dout = inputs(name)
    t2, d2 = t[[0, -1]], dout[[0, -1]].contiguous()
    out, gy0, gp = run(m, y0, t2, d2, adjoint_params)
    want = run(m, y0, t2, d2, adjoint_params,
               entry=lambda m, yy, t: odeint_adjoint(m, yy, t, method="dopri5", adjoint_params=adjoint_params))
    assert len(attempts_of(m)) == 1
    assert torch.equal(out, want[0])
    assert torch.equal(gy0, want[1])
    if adjoint_params is None:
        ps = list(m.parameters())
        off = np.cumsum([0] + [p.numel() for p in ps])
        for i, p in enumerate(ps):
            assert torch.equal(gp[off[i]:off[i + 1]], want[2][off[i]:off[i + 1]]), "parameter %d" % i
    else:
        assert gp is None and want[2] is None


@pytest.mark.parametrize("name", A.NAMES)
def test_values_are_odeint_denses(name):
    from nlbac_amd.ode_dense import odeint_dense, odeint_dense_adjoint
    c, m, y0, t, dout = inputs(name)
    ns = c["n_s"]
    yy = y0.clone().requires_grad_(True)
    out = odeint_dense_adjoint(m, yy, t)
    assert out.requires_grad and out.shape == (len(t), y0.shape[0], y0.shape[1])
    assert torch.equal(out.detach(), odeint_dense(m, y0.clone().requires_grad_(True), t).detach())
    with torch.no_grad():
        assert torch.equal(out.detach(), odeint_dense(m, y0, t))
        quiet = odeint_dense_adjoint(m, y0, t)
    assert torch.equal(out.detach(), quiet) and not quiet.requires_grad
    assert torch.equal(out[0].detach(), y0)
    for j in range(1, len(t)):
        assert torch.equal(out[j][:, ns:].detach(), y0[:, ns:]), "carried columns of out[%d]" % j
        vec_close(out[j].detach().cpu().numpy(), c["out"][j].numpy(), TOL, "%s out[%d]" % (name, j))


@pytest.mark.parametrize("name", A.NAMES)
def test_input_gradients_match_the_reference(name):
    """``adjoint_params=()``: every interval's adjoint solve takes the reference's number of attempts (the cases hold no
    decision within 0.25 of the threshold), and d/dy0 then agrees to 1e-4 — on the state and on the carried columns,
    whose output gradients are summed outside the solves (``dout`` is nonzero on every point and column)."""
    c, m, y0, t, dout = inputs(name)
    ns = c["n_s"]
    r = A.adjoint(name, False)
    assert bool((c["dout"] != 0).all())
    out, gy0, gp = run(m, y0, t, dout, ())
    dev = attempts_of(m)
    print("%s: attempts per interval, last first: device %s, reference %s" % (name, dev, r["attempts"]))
    assert dev == r["attempts"] == A.WANT_ATTEMPTS[name]
    e = vec_close(gy0[:, :ns].cpu().numpy(), r["gy0"][:, :ns].numpy(), TOL, "%s d/dx0" % name)
    f = vec_close(gy0[:, ns:].cpu().numpy(), r["gy0"][:, ns:].numpy(), TOL, "%s d/d carried" % name)
    print("%s: d/dx0 %.3g, d/d carried %.3g of scale" % (name, e, f))
    assert gp is None


@pytest.mark.parametrize("name", A.NAMES)
def test_parameter_adjoint_matches_the_reference(name):
    """``adjoint_params=None``, by ``test_adjoint_gpu``'s rule: the parameter adjoint's error estimate carries ReLU-kink
    noise, the sequences are long and hold marginal decisions (the reference's own: ratios 0.994 and 1.048 in the Unicycle
    case, 0.917 in the other).  Where every interval took the reference's number of attempts: d/dy0 at 1e-4 and the
    parameter gradient's relative L2 error below 1e-3; otherwise both are valid dopri5 runs that agree to solver tolerance,
    5e-3 — three times the 1.7e-3 measured between neighbouring valid runs of the reference (rtol x 1.02, x 0.98, float64)."""
    c, m, y0, t, dout = inputs(name)
    ns = c["n_s"]
    r = A.adjoint(name, True)
    out, gy0, gp = run(m, y0, t, dout, None)
    dev = attempts_of(m)
    same = dev == r["attempts"]
    tol, bar = (TOL, 1e-3) if same else (5e-3, 5e-3)
    l2 = A.rel_l2(gp.cpu().numpy(), r["gp"].numpy())
    print("%s: attempts per interval, last first: device %s, reference %s -> %s branch (d/dy0 at %.0e, theta at %.0e); "
          "theta rel L2 %.3g" % (name, dev, r["attempts"], "same-sequence" if same else "other-sequence", tol, bar, l2))
    e = vec_close(gy0[:, :ns].cpu().numpy(), r["gy0"][:, :ns].numpy(), tol, "%s d/dx0" % name)
    f = vec_close(gy0[:, ns:].cpu().numpy(), r["gy0"][:, ns:].numpy(), tol, "%s d/d carried" % name)
    print("%s: d/dx0 %.3g, d/d carried %.3g of scale" % (name, e, f))
    assert l2 < bar


@pytest.mark.parametrize("name", A.NAMES)
def test_against_the_direct_backward_on_the_device(name):
    """The continuous adjoint against ``odeint_dense``'s back-propagation through the accepted steps under the same
    ``dout``: solver tolerance (``test_adjoint_gpu``'s dopri5 bar for T < 0.1) on d/dy0; the parameter gradients'
    distance is printed beside the reference's own (adjoint vs direct on the CPU: 1.9e-2 Unicycle, 7.3e-3 SimulatedCars)."""
    from nlbac_amd.ode_dense import odeint_dense
    c, m, y0, t, dout = inputs(name)
    _, gy0, gp = run(m, y0, t, dout, None)
    _, gy0_d, gp_d = run(m, y0, t, dout, None, entry=odeint_dense)
    e = A.rel_l2(gy0.cpu().numpy(), gy0_d.cpu().numpy())
    ref = A.rel_l2(A.adjoint(name, True)["gp"].numpy(), c["gp_direct"].numpy())
    print("%s: adjoint vs direct on the device: d/dy0 rel L2 %.3g; theta rel L2 %.3g (the reference's own: %.3g)"
          % (name, e, A.rel_l2(gp.cpu().numpy(), gp_d.cpu().numpy()), ref))
    assert e < 5e-3


@pytest.mark.parametrize("kind", ["affine 160", "single-net staged"])
def test_the_other_adjoint_step_paths_are_served(kind):
    """Whatever serves a one-interval adjoint serves the walk: the 160-wide control-affine NODE (the LDS-tiled step
    kernel, interpolation as a launch of its own) and the single-net NODE stage by stage (``adj_fused = False``).  Two
    points: ``odeint_adjoint``'s bits; on a grid: the direct gradient of the same solve to solver tolerance."""
    from nlbac_amd import ode_dense
    from nlbac_amd.odeint import _solver_of, odeint_adjoint
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6, hidden_dim=160) if kind == "affine 160" else NeuralODEModel(12, 10)
    width = 5 if kind == "affine 160" else 12
    gen = torch.Generator().manual_seed(4)
    y0 = (torch.rand(70, width, generator=gen) * 2 - 1).cuda()
    t = torch.tensor([0.0, 0.01, 0.03, 0.06])
    dout = (torch.randn(len(t), 70, width, generator=gen) / 70).cuda()
    if kind != "affine 160":
        m.device_handles()
        ode_dense.solver_of(m, ode_dense.ADJOINT).adj_fused = False
        _solver_of(m, True).adj_fused = False
    t2, d2 = t[[0, -1]], dout[[0, -1]].contiguous()
    got = run(m, y0, t2, d2)
    want = run(m, y0, t2, d2, entry=lambda m, yy, t: odeint_adjoint(m, yy, t, method="dopri5"))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    _, gy0, gp = run(m, y0, t, dout)
    _, gy0_d, gp_d = run(m, y0, t, dout, entry=ode_dense.odeint_dense)
    e = A.rel_l2(gy0.cpu().numpy(), gy0_d.cpu().numpy())
    print("%s: attempts %s; adjoint vs direct d/dy0 rel L2 %.3g, theta rel L2 %.3g"
          % (kind, attempts_of(m), e, A.rel_l2(gp.cpu().numpy(), gp_d.cpu().numpy())))
    assert e < 5e-3


@pytest.mark.parametrize("name", A.NAMES)
def test_two_calls_give_the_same_bits(name):
    c, m, y0, t, dout = inputs(name)
    a, b = run(m, y0, t, dout), run(m, y0, t, dout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_backward_after_another_solve_is_refused():
    from nlbac_amd.ode_dense import odeint_dense_adjoint
    c, m, y0, t, dout = inputs("unicycle")
    first = odeint_dense_adjoint(m, y0.clone().requires_grad_(True), t)
    second = odeint_dense_adjoint(m, y0.clone().requires_grad_(True), t)
    with pytest.raises(AssertionError, match="backward must run before the next odeint_dense_adjoint"):
        (first * dout).sum().backward()
    (second * dout).sum().backward()


@pytest.mark.parametrize("name", A.NAMES)
def test_the_other_entries_solvers_are_left_alone(name):
    from nlbac_amd import ode_dense
    from nlbac_amd.odeint import odeint, odeint_adjoint
    c, m, y0, t, dout = inputs(name)
    t2, d2 = t[[0, 2]], dout[[0, 2]].contiguous()
    run(m, y0, t2, d2, entry=lambda m, yy, t: odeint(m, yy, t, method="dopri5"))
    run(m, y0, t2, d2, entry=lambda m, yy, t: odeint_adjoint(m, yy, t, method="dopri5"))
    run(m, y0, t, dout, entry=ode_dense.odeint_dense)
    others = [m._odeint_solver, m._odeint_solver_adj] + [sv for k, sv in m.__dict__[ode_dense.SOLVERS_KEY].items()
                                                         if k != ode_dense.ADJOINT]
    state = lambda: [(sv._chain_len, sv._adj_chain, sv.stats["solves"], {k: p.n_slots for k, p in sv._pools.items()})
                     for sv in others]
    before = state()
    run(m, y0, t, dout)
    mine = ode_dense.solver_of(m, ode_dense.ADJOINT)
    assert all(sv is not mine for sv in others) and len(others) >= 3
    assert mine.adjoint and not mine.keep_acts and not mine.interp_fold
    assert state() == before


def test_what_is_not_served_raises(monkeypatch):
    from nlbac_amd import ode_dense
    c, m, y0, t, dout = inputs("unicycle")
    sv = ode_dense.solver_of(m, ode_dense.ADJOINT)
    monkeypatch.setattr(sv, "device_loop", False)
    with pytest.raises(NotImplementedError, match="_chain_ok.*device_loop=False"):
        ode_dense.odeint_dense_adjoint(m, y0, t)
    monkeypatch.undo()
    solves = sv.stats["solves"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="hipGraph capture"):
        ode_dense.odeint_dense_adjoint(m, y0, t)
    monkeypatch.undo()
    assert sv.stats["solves"] == solves, "a refused call ran a solve"

    class Two:
        world = 2
    out = ode_dense.odeint_dense_adjoint(m, y0.clone().requires_grad_(True), t)
    monkeypatch.setattr(sv, "comm", Two())
    with pytest.raises(NotImplementedError, match="sample-sharded"):
        (out * dout).sum().backward()


def _r512(nbytes):
    return -(-nbytes // 512) * 512


@pytest.mark.parametrize("name", A.NAMES)
def test_a_forward_holds_the_outputs_and_the_carried_columns(name):
    """After a warm-up call (the slot pool, the scratch buffers and the previous solve's state and carried columns are the
    solver's), a forward with gradients enabled adds ``out`` and at most the carried columns to what is allocated —
    nothing that grows with the accepted steps or the grid — on the 5-point grid and on a 9-point grid over the same
    span alike, and strictly less than ``odeint_dense`` adds there."""
    from nlbac_amd.ode_dense import odeint_dense, odeint_dense_adjoint
    c, m, y0, t, dout = inputs(name)
    ns = c["n_s"]
    t9 = torch.linspace(float(t[0]), float(t[-1]), 9)
    c_bytes = _r512(y0.shape[0] * (y0.shape[1] - ns) * 4)

    def added(entry, grid):
        yy = y0.clone().requires_grad_(True)
        o = entry(m, yy, grid)                       # warm-up
        (o * torch.ones_like(o)).sum().backward()
        del o
        yy.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        o = entry(m, yy, grid)
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - base
        return grown, _r512(o.numel() * 4)

    extra = {}
    for label, grid in (("5 points", t), ("9 points", t9)):
        grown, out_bytes = added(odeint_dense_adjoint, grid)
        dense, _ = added(odeint_dense, grid)
        print("%s, %s: the forward adds %d bytes (out %d, carried columns %d); odeint_dense adds %d"
              % (name, label, grown, out_bytes, c_bytes, dense))
        assert out_bytes <= grown <= out_bytes + c_bytes
        assert grown < dense
        extra[label] = grown - out_bytes
    assert extra["5 points"] == extra["9 points"]


@pytest.mark.parametrize("n", [1, 37, 300])
@pytest.mark.parametrize("ns,nu", [(3, 2), (10, 2)])
def test_the_restart_kernel_alone(n, ns, nu):
    """``nlbac_adj_dense_restart`` through the binding: y and dout read in place from padded rows, with the state of the
    interval above and without (NULL: ``nlbac_adj_pack``'s result)."""
    from nlbac_amd import _lib
    from nlbac_amd.arena import stream_ptr
    gen = torch.Generator().manual_seed(100 * n + ns)
    W, y_ld, d_ld = 2 * ns + nu, ns + nu + 3, ns + nu + 5
    y = torch.randn(n, y_ld, generator=gen).cuda()
    d = torch.randn(n, d_ld, generator=gen).cuda()
    zp = torch.randn(n, W, generator=gen).cuda()
    z0 = torch.full((n + 1, W), 7.0, device="cuda")                    # (one guard row behind the last)
    _lib.call("nlbac_adj_dense_restart", y.data_ptr(), y_ld, d.data_ptr(), d_ld, zp.data_ptr(), ns, nu, n, z0.data_ptr(),
              stream_ptr())
    want = torch.cat([y[:, :ns], zp[:, ns:2 * ns] + d[:, :ns], zp[:, 2 * ns:]], 1)
    assert torch.equal(z0[:n], want) and bool((z0[n] == 7.0).all())
    z0.fill_(7.0)
    _lib.call("nlbac_adj_dense_restart", y.data_ptr(), y_ld, d.data_ptr(), d_ld, None, ns, nu, n, z0.data_ptr(),
              stream_ptr())
    want = torch.cat([y[:, :ns], d[:, :ns], torch.zeros(n, nu, device="cuda")], 1)
    assert torch.equal(z0[:n], want) and bool((z0[n] == 7.0).all())
    packed = torch.full((n, W), 7.0, device="cuda")
    yc, dc = y[:, :ns].contiguous(), d[:, :ns].contiguous()
    _lib.call("nlbac_adj_pack", yc.data_ptr(), dc.data_ptr(), ns, nu, n, packed.data_ptr(), stream_ptr())
    assert torch.equal(z0[:n], packed)
