"""GPU: ``nlbac_amd.ode_dense.odeint_dense`` — one adaptive dopri5 solve read at every point of a time grid — against
the CPU reference composed from the oracle's pieces (``dense_common``: values, gradients w.r.t. the state, the carried
columns and the parameters), against ``odeint`` where the two must coincide (two time points; an output gradient at the
last point only), and against itself (linearity in the output gradient, determinism, a solver state of its own).

Two width-64 NODEs: the Unicycle one on 200 rows (ragged against the 32-row tile; five accepted steps holding 2, 1, 0, 3
and 1 outputs — more steps than a slot pool starts with, so the solve is restarted once in a larger pool) and the
single-net SimulatedCars one on 64 rows (three steps holding 2, 0 and 3 outputs)."""
import functools

import numpy as np
import pytest
import torch

import dense_common as D
from common import vec_close
from test_agent_parity_gpu import make_agent
from test_solver_gpu import rows_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAMES = ["unicycle", "cars"]


@functools.lru_cache(maxsize=None)
def _agent(name):
    env = D.CASES[name]["env"]
    return make_agent(64, 64, 0, "dopri5") if env == "Unicycle" else make_agent(64, 64, 0, "dopri5", env)


def node_of(name):
    m = _agent(name)[0].neural_ode_model
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def grads(m, y0, t, dout, params=True, **kw):
    """(out, d/dy0, flat d/d theta or None) of ``sum(out * dout)``."""
    from nlbac_amd.ode_dense import odeint_dense
    yy = y0.clone().requires_grad_(True)
    out = odeint_dense(m, yy, t, **kw)
    ps = list(m.parameters()) if params else []
    g = torch.autograd.grad((out * dout).sum(), [yy] + ps)
    return out.detach(), g[0], (torch.cat([v.reshape(-1) for v in g[1:]]) if params else None)


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("name", NAMES)
def test_values_and_gradients_match_the_reference(name):
    from nlbac_amd import ode_dense
    c = D.case(name)
    m, ns = node_of(name), c["n_s"]
    y0, t, dout = c["y0"].cuda(), c["t"], c["dout"].cuda()
    out, gy0, gp = grads(m, y0, t, dout)
    # the device took the reference's steps, and no output sits where a step size's fp32 noise could move it to a neighbour
    sv = ode_dense.solver_of(m, "params")
    dev = [a[0] for a in sv.ctx["info"] if a[0] is not None]
    assert [d[2] for d in dev] == [s[2] for s in c["steps"]], (dev, c["steps"])
    np.testing.assert_allclose([d[0] for d in dev], [s[0] for s in c["steps"]], rtol=2e-3)
    assert sv.ctx["nacc"] == [len(c["ends"]) - 1] and len(sv.ctx["steps"]) == len(c["ends"])
    taus = ode_dense._taus(t)
    ends = np.cumsum([d[0] for d in dev if d[2]])
    gap = min(abs(e - x) for e in ends for x in taus)
    print("%s: nearest accepted-step end to an output time: %.4g (bar %.4g)" % (name, gap, 2e-3 * taus[-1]))
    assert gap > 2e-3 * taus[-1]
    assert D.outputs_per_step(list(ends), D.times_of(t)) == c["want_per_step"]
    # values
    assert out.shape == c["out"].shape
    assert torch.equal(out[0], y0)
    for j in range(1, len(t)):
        e = vec_close(out[j].cpu().numpy(), c["out"][j].numpy(), TOL, "%s out[%d]" % (name, j))
        print("%s: out[%d] vs the reference: %.3g of scale" % (name, j, e))
        assert torch.equal(out[j][:, ns:], y0[:, ns:]), "carried columns of out[%d]" % j
    # gradients: the fp64 run's kink margin decides which rows may leave the bar (test_solver_gpu.rows_close)
    near, off = rows_close(gy0[:, :ns].cpu().numpy(), c["gy0"][:, :ns].numpy(), "%s d/dx0" % name, c["margin"])
    print("%s: d/dx0: %d rows near a kink, %d beyond %.0e" % (name, near, off, TOL))
    near, off = rows_close(gy0[:, ns:].cpu().numpy(), c["gy0"][:, ns:].numpy(), "%s d/d carried" % name, c["margin"])
    print("%s: d/d carried: %d rows near a kink, %d beyond %.0e" % (name, near, off, TOL))
    a, b = gp.cpu().numpy().astype(np.float64), c["gp"].numpy().astype(np.float64)
    l2 = np.linalg.norm(a - b) / np.linalg.norm(b)
    far = (np.abs(a - b) > 1e-3 * np.abs(b).max()).mean()
    print("%s: d/d theta: relative L2 error %.3e, %.3g %% of the entries beyond 1e-3 of the largest" % (name, l2, 100 * far))
    assert l2 <= 5e-3 and far <= 0.01


@pytest.mark.parametrize("name", NAMES)
def test_a_gradient_at_the_last_point_alone_is_odeints(name):
    """The same steps and the same backward launches per step as ``odeint`` over [t[0], t[-1]] (whose chain carries the
    gradients between its launches itself): the same bits."""
    from nlbac_amd.odeint import odeint
    c = D.case(name)
    m, ns = node_of(name), c["n_s"]
    y0, t = c["y0"].cuda(), c["t"]
    dout = torch.zeros_like(c["dout"])
    dout[-1, :, :ns] = c["dout_last"]
    dout[-1, :, ns:] = c["dout"][-1, :, ns:]
    dout = dout.cuda()
    out, gy0, gp = grads(m, y0, t, dout)
    yy = y0.clone().requires_grad_(True)
    o2 = odeint(m, yy, t[[0, -1]], method="dopri5")
    g2 = torch.autograd.grad((o2[-1] * dout[-1]).sum(), [yy] + list(m.parameters()))
    gp2 = torch.cat([v.reshape(-1) for v in g2[1:]])
    assert torch.equal(out[-1], o2[-1].detach())
    print("%s: last-point gradient vs odeint: d/dy0 %.3g, d/d theta %.3g of scale" % (name, rel(gy0, g2[0]), rel(gp, gp2)))
    # (measured on an MI355X: zero in both cases — a slot without an output of its own gets zeros, and adding what the
    #  next step sends back to zeros is what the chain's carry does)
    assert torch.equal(gy0, g2[0]) and torch.equal(gp, gp2)


@pytest.mark.parametrize("name", NAMES)
def test_the_gradient_is_linear_in_the_output_gradient(name):
    """d/d(y0, theta) under ``dout`` = the sum over the output points of the gradients under ``dout`` restricted to one
    point: the per-slot sums of the injection launch and the carries between the steps, re-associated in fp32."""
    from nlbac_amd.ode_dense import odeint_dense
    c = D.case(name)
    m = node_of(name)
    y0, t, dout = c["y0"].cuda(), c["t"], c["dout"].cuda()
    yy = y0.clone().requires_grad_(True)
    out = odeint_dense(m, yy, t)
    wrt = [yy] + list(m.parameters())
    flat = lambda g: (g[0], torch.cat([v.reshape(-1) for v in g[1:]]))
    whole = flat(torch.autograd.grad((out * dout).sum(), wrt, retain_graph=True))
    parts = None
    for j in range(len(t)):
        g = flat(torch.autograd.grad((out[j] * dout[j]).sum(), wrt, retain_graph=True))
        parts = g if parts is None else (parts[0] + g[0], parts[1] + g[1])
    e0, e1 = rel(parts[0], whole[0]), rel(parts[1], whole[1])
    print("%s: sum of single-point gradients vs the whole: d/dy0 %.3g, d/d theta %.3g of scale" % (name, e0, e1))
    assert e0 <= 1e-5 and e1 <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_two_points_are_odeint_itself(name):
    from nlbac_amd.ode_dense import odeint_dense
    from nlbac_amd.odeint import odeint
    c = D.case(name)
    m = node_of(name)
    y0, t = c["y0"].cuda(), c["t"][[0, -1]]
    with torch.no_grad():
        a, b = odeint_dense(m, y0, t), odeint(m, y0, t, method="dopri5")
    assert a.shape == b.shape and torch.equal(a[-1], b[-1]) and torch.equal(a[0], b[0])
    yy = y0.clone().requires_grad_(True)
    assert torch.equal(odeint_dense(m, yy, t)[-1].detach(), b[-1])      # (what is kept does not change the values)
    tl = [float(v) for v in t]                                          # a Python sequence is rounded as odeint rounds it
    with torch.no_grad():
        assert torch.equal(odeint_dense(m, y0, tl)[-1], odeint(m, y0, tl, method="dopri5")[-1])


def test_without_gradients_nothing_is_kept():
    from nlbac_amd.ode_dense import odeint_dense
    c = D.case("unicycle")
    m = node_of("unicycle")
    y0 = c["y0"].cuda().requires_grad_(True)
    with torch.no_grad():
        out = odeint_dense(m, y0, c["t"])
    assert not out.requires_grad and out.grad_fn is None
    with pytest.raises(RuntimeError):
        out.sum().backward()
    ref, _, _ = grads(m, c["y0"].cuda(), c["t"], c["dout"].cuda())
    assert torch.equal(out, ref)


@pytest.mark.parametrize("name", NAMES)
def test_input_gradients_alone_keep_mask_words(name):
    """Parameters that need no gradient: the solver keeps ReLU mask words, not activation rows (a solver of its own per
    keep mode), and the input gradients are those of the run that keeps the rows, to fp32 re-association."""
    from nlbac_amd import ode_dense
    c = D.case(name)
    m = node_of(name)
    y0, t, dout = c["y0"].cuda(), c["t"], c["dout"].cuda()
    out_p, gy0_p, _ = grads(m, y0, t, dout)
    for p in m.parameters():
        p.requires_grad_(False)
    try:
        out_i, gy0_i, _ = grads(m, y0, t, dout, params=False)
    finally:
        for p in m.parameters():
            p.requires_grad_(True)
    sv_i, sv_p = ode_dense.solver_of(m, "inputs"), ode_dense.solver_of(m, "params")
    assert sv_i is not sv_p and not sv_i.keep_acts and sv_p.keep_acts
    # (the one-step kernels sum f_net's output layer in two parts when they keep words only — see rollout: the values
    #  may differ in the last bits, 6e-8 per operation over a few hundred operations, and a row next to a ReLU kink may
    #  then take the other branch: rows_close's bars, as against the reference)
    e_out = rel(out_i, out_p)
    print("%s: mask words vs rows: out %.3g of scale" % (name, e_out))
    assert e_out <= 1e-5
    ns = c["n_s"]
    rows_close(gy0_i[:, :ns].cpu().numpy(), gy0_p[:, :ns].cpu().numpy(), "%s d/dx0, words vs rows" % name, c["margin"])
    rows_close(gy0_i[:, ns:].cpu().numpy(), gy0_p[:, ns:].cpu().numpy(), "%s d/d carried, words vs rows" % name, c["margin"])


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_give_the_same_bits(name):
    c = D.case(name)
    m = node_of(name)
    y0, t, dout = c["y0"].cuda(), c["t"], c["dout"].cuda()
    a, b = grads(m, y0, t, dout), grads(m, y0, t, dout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("name", NAMES)
def test_odeints_solver_is_left_alone(name):
    from nlbac_amd import ode_dense
    from nlbac_amd.odeint import odeint
    c = D.case(name)
    m = node_of(name)
    y0, t = c["y0"].cuda(), c["t"]

    def run():
        yy = y0.clone().requires_grad_(True)
        o = odeint(m, yy, t[[0, 2]], method="dopri5")
        return o.detach(), torch.autograd.grad((o[-1] * c["dout"][2].cuda()).sum(), yy)[0]
    before = run()
    chain_len = m._odeint_solver._chain_len
    grads(m, y0, t, c["dout"].cuda())
    assert m._odeint_solver._chain_len == chain_len
    assert all(sv is not m._odeint_solver for sv in m.__dict__[ode_dense.SOLVERS_KEY].values())
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_what_is_not_served_raises(monkeypatch):
    from nlbac_amd import ode_dense
    c = D.case("unicycle")
    m = node_of("unicycle")
    y0, t = c["y0"].cuda(), c["t"]
    sv = ode_dense.solver_of(m, "none")
    monkeypatch.setattr(sv, "device_loop", False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="_chain_ok.*device_loop=False"):
        ode_dense.odeint_dense(m, y0, t)
    monkeypatch.undo()
    solves = sv.stats["solves"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="hipGraph capture"):
        ode_dense.odeint_dense(m, y0, t)
    assert sv.stats["solves"] == solves, "a refused call ran a solve"
