"""GPU: ``rollout(..., step_size=s)`` — every control interval solved in steps of ``s`` with its control held, one launch
forward and one backward (``nlbac_*_rk_hold_*``) — against the chain of ``odeint(..., options=dict(step_size=s))`` calls
written out with autograd through the chain, against ``odeint_grid`` (H = 1), against ``rollout`` without ``step_size``
(m = 1), and the one launch against the chained path (``ONE_LAUNCH`` off); launch counts; what the forward keeps.

Bounds.  States, d/dx0 and d/dcontrols are the same fp32 operations in the same order on both sides: ``torch.equal``.
Parameter gradients differ in fp32 summation order only (one weight-gradient launch over all H * m * stages * rows
against one per call, resp. per fine interval): ||a - b|| <= 1e-5 ||b|| per tensor, the bar of
``test_one_launch_equals_chain``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"unicycle": (3, 3, 6), "pvtol": (6, 6, 12), "cars": (12, 10)}
KINDS = ["unicycle", "pvtol", "cars"]
SCHEDULES = [(0.05, 0.02), (1 / 8, 1 / 32)]      # m = 3 with a short last step; m = 4, all steps equal
MODES = ("none", "inputs", "params")
H = 3
PARAM_BAR = 1e-5


def make(kind, seed=0, **kw):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(seed)
    m = NeuralODEModel(*SHAPES[kind], **kw)
    return m, m.n_s, (m.n_u if m.affine else m.n_carry)


def inputs(ns, nc, B, H, seed=3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, ns, generator=g) * 2 - 1
    c = torch.rand(H, B, nc, generator=g) * 2 - 1
    return x0.cuda(), c.cuda()


def weights(T, B, ns, seed=5):
    return torch.randn(T, B, ns, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.fixture
def one_launch():
    from nlbac_amd import rollout as R
    old = R.ONE_LAUNCH
    yield R
    R.ONE_LAUNCH = old


def spy(monkeypatch):
    from nlbac_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def run(m, mode, x0, c, w, solve):
    """``solve(x, u)`` -> out under keep-mode ``mode`` with the loss (out * w).sum():
    (out, d/dx0, d/dcontrols, parameter gradients)."""
    for p in m.parameters():
        p.requires_grad_(mode == "params")
    m.zero_grad()
    if mode == "none":
        with torch.no_grad():
            return solve(x0, c), None, None, []
    x, u = x0.clone().requires_grad_(), c.clone().requires_grad_()
    out = solve(x, u)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, u.grad, [p.grad.clone() for p in m.parameters()] if mode == "params" else []


def held(m, dt, method, s):
    from nlbac_amd.rollout import rollout
    return lambda x, u: rollout(m, x, u, dt, method=method, step_size=s)


def chain(m, ns, dt, method, s, fresh_solvers=False):
    """The chain the docstring of ``rollout`` writes out: one ``odeint`` call with ``options=dict(step_size=s)`` per
    control interval, autograd through the chain.  ``fresh_solvers`` (nets on ``odeint_grid``'s chained path, whose
    per-interval solvers are cached on the model and serve one live solve at a time): each call gets solvers of its
    own, so that all H calls can be differentiated afterwards."""
    from nlbac_amd.odeint import odeint

    def solve(x, u):
        t, outs = torch.tensor([0.0, dt]), [x]
        for k in range(u.shape[0]):
            if fresh_solvers:
                m.__dict__.pop("_odeint_subgrid_solvers", None)
            x = odeint(m, torch.cat([x, u[k]], 1), t, method=method, options=dict(step_size=s))[-1][:, :ns]
            outs.append(x)
        return torch.stack(outs)
    return solve


def same(m, got, ref, tag):
    """States and input gradients bit for bit, parameter gradients at PARAM_BAR."""
    (o1, gx1, gc1, gp1), (o0, gx0, gc0, gp0) = got, ref
    assert o1.shape == o0.shape and torch.equal(o1, o0), "%s: states" % tag
    assert (gx1 is None) == (gx0 is None) and len(gp1) == len(gp0)
    if gx1 is not None:
        assert torch.equal(gx1, gx0), "%s: d/dx0" % tag
        assert gc1.shape == gc0.shape and torch.equal(gc1, gc0), "%s: d/dcontrols" % tag
    errs = {}
    for (name, _), a, b in zip(m.named_parameters(), gp1, gp0):
        errs[name] = float((a - b).norm()) / max(1e-12, float(b.norm()))
    if errs:
        print("%s: parameter gradients, ||a - b|| / ||b||: %s" % (tag, "  ".join("%s %.3g" % kv for kv in errs.items())))
    for name, e in errs.items():
        assert e <= PARAM_BAR, "%s: d/d%s %.3g" % (tag, name, e)


def check_against_odeint_chain(m, ns, nc, method, B, dt, s, modes, tag, fresh_solvers=False):
    x0, c = inputs(ns, nc, B, H)
    w = weights(H + 1, B, ns)
    for mode in modes:
        got = run(m, mode, x0, c, w, held(m, dt, method, s))
        assert got[0].shape == (H + 1, B, ns) and torch.equal(got[0][0], x0)
        ref = run(m, mode, x0, c, w, chain(m, ns, dt, method, s, fresh_solvers))
        same(m, got, ref, "%s %s dt=%g s=%g B=%d %s" % (tag, method, dt, s, B, mode))
    return got


# ---- 1. the chain of odeint(..., options=dict(step_size=s)) calls
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
@pytest.mark.parametrize("dt,s", SCHEDULES)
def test_equals_chain_of_odeint_with_step_size(kind, method, B, dt, s):
    m, ns, nc = make(kind)
    check_against_odeint_chain(m, ns, nc, method, B, dt, s, MODES, kind)


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_equals_chain_of_odeint_with_step_size_many_tiles(kind):
    m, ns, nc = make(kind)
    check_against_odeint_chain(m, ns, nc, "rk4", 8192, 0.05, 0.02, ("params",), kind)


def test_sub_steps_are_not_one_step():
    """(the option does something: three euler steps over a control interval are not one)"""
    from nlbac_amd.rollout import rollout
    m, ns, nc = make("unicycle")
    x0, c = inputs(ns, nc, 40, H)
    with torch.no_grad():
        a, b = rollout(m, x0, c, 0.05, method="euler", step_size=0.02), rollout(m, x0, c, 0.05, method="euler")
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1:], b[1:])


# ---- 2. one control interval: odeint_grid on t = [0, dt] under step_size
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
@pytest.mark.parametrize("dt,s", SCHEDULES)
def test_one_interval_equals_odeint_grid(kind, method, B, dt, s):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    x0, c = inputs(ns, nc, B, 1)
    w = weights(2, B, ns)
    grid = lambda x, u: odeint_grid(m, torch.cat([x, u[0]], 1), torch.tensor([0.0, dt]), method=method, step_size=s)[:, :, :ns]
    for mode in MODES:
        same(m, run(m, mode, x0, c, w, held(m, dt, method, s)), run(m, mode, x0, c, w, grid),
             "%s %s dt=%g s=%g B=%d %s" % (kind, method, dt, s, B, mode))


# ---- 3. m = 1: rollout without step_size
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
@pytest.mark.parametrize("s", ["dt", 1.0])
def test_one_fine_step_equals_rollout_without_step_size(kind, method, B, s):
    from nlbac_amd.ode_grid import _sub_grid
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    dt = 0.02      # (float32(0.02) < 0.02: a step_size of dt is one fine step; float32(0.05) > 0.05 would leave a second one)
    s = dt if s == "dt" else s
    assert len(_sub_grid(torch.tensor([0.0, dt]), s)[1]) == 1
    x0, c = inputs(ns, nc, B, H)
    w = weights(H + 1, B, ns)
    plain = lambda x, u: rollout(m, x, u, dt, method=method)
    for mode in MODES:
        same(m, run(m, mode, x0, c, w, held(m, dt, method, s)), run(m, mode, x0, c, w, plain),
             "%s %s s=%g B=%d %s" % (kind, method, s, B, mode))


# ---- 4. the one launch against the chained path
def check_one_launch_against_chained(R, monkeypatch, kind, method, B, dt, s, mode):
    m, ns, nc = make(kind)
    x0, c = inputs(ns, nc, B, H)
    w = weights(H + 1, B, ns)
    calls = spy(monkeypatch)
    R.ONE_LAUNCH = True
    one = run(m, mode, x0, c, w, held(m, dt, method, s))
    assert [n for n in calls if "_hold_" in n], calls
    del calls[:]
    R.ONE_LAUNCH = False
    chained = run(m, mode, x0, c, w, held(m, dt, method, s))
    assert calls and not [n for n in calls if "_hold_" in n or "_traj_" in n or "_grid_" in n or "_subgrid_" in n], calls
    same(m, one, chained, "%s %s dt=%g s=%g B=%d %s, one launch vs chained" % (kind, method, dt, s, B, mode))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("dt,s", SCHEDULES)
@pytest.mark.parametrize("mode", ["inputs", "params"])
def test_one_launch_equals_chained_path(one_launch, monkeypatch, kind, method, dt, s, mode):
    check_one_launch_against_chained(one_launch, monkeypatch, kind, method, 96, dt, s, mode)


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_one_launch_equals_chained_path_many_tiles(one_launch, monkeypatch, kind):
    check_one_launch_against_chained(one_launch, monkeypatch, kind, "rk4", 8192, 0.05, 0.02, "params")


# ---- 5. the normalised single-net NODE
def test_normalised_net():
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    g = torch.Generator().manual_seed(11)
    r = lambda n, lo, hi: (torch.rand(n, generator=g) * (hi - lo) + lo).numpy()
    torch.manual_seed(0)
    m = NeuralODEModel(8, 6, normalizer=(r(8, -0.5, 0.5), r(8, 0.5, 2.0), r(6, -0.3, 0.3), r(6, 0.5, 2.0)))
    for dt, s in SCHEDULES:
        check_against_odeint_chain(m, m.n_s, m.n_carry, "rk4", 96, dt, s, ("params",), "quadrotor")


# ---- 6. a net the register-resident kernels refuse
@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_wide_net_takes_the_chained_path(monkeypatch, kind):
    from nlbac_amd import rollout as R
    m, ns, nc = make(kind, hidden_dim=160)
    assert R.ONE_LAUNCH and not R._one_launch_ok(m, "rk4")
    x0, c = inputs(ns, nc, 40, H)
    calls = spy(monkeypatch)
    with torch.no_grad():
        R.rollout(m, x0, c, 0.05, method="rk4", step_size=0.02)
    assert calls and not [n for n in calls if "_hold_" in n or "_traj_" in n or "_grid_" in n or "_subgrid_" in n], calls
    for dt, s in SCHEDULES:
        check_against_odeint_chain(m, ns, nc, "rk4", 40, dt, s, MODES, kind + " hidden 160", fresh_solvers=True)


# ---- 7. launch counts
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("params", [False, True])
def test_hold_launch_counts(one_launch, monkeypatch, kind, method, params):
    m, ns, nc = make(kind)
    for p in m.parameters():
        p.requires_grad_(params)
    x0, c = inputs(ns, nc, 96, H)
    c.requires_grad_()
    one_launch.ONE_LAUNCH = True
    calls = spy(monkeypatch)
    out = one_launch.rollout(m, x0, c, 0.05, method=method, step_size=0.02)
    fam = "nlbac_node_rk" if m.affine else "nlbac_concat_rk"
    assert [n for n in calls if n.startswith(("nlbac_node_rk", "nlbac_concat_rk"))] == [fam + "_hold_fwd"], calls
    del calls[:]
    out.sum().backward()
    assert calls == [fam + "_hold_bwd"] + (["nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"] if params else []), calls
    assert c.grad.shape == c.shape


# ---- 8. what the forward keeps does not scale with the fine states
@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_input_grads_keep_no_rows(one_launch, kind):
    m, ns, nc = make(kind)
    B, Hc, mf, S = 8192, 4, 4, 4
    dt, s = 1 / 8, 1 / 32
    x0, c = inputs(ns, nc, B, Hc)
    for p in m.parameters():
        p.requires_grad_(False)
    c.requires_grad_()
    one_launch.ONE_LAUNCH = True
    one_launch.rollout(m, x0, c, dt, method="rk4", step_size=s).sum().backward()       # warm-up: caches, weight packs
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = one_launch.rollout(m, x0, c, dt, method="rk4", step_size=s)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert out.shape == (Hc + 1, B, ns)
    # per (fine interval, stage, row): the affine form's G and its two nets' seven layers of mask words, 16 B each; the
    # single-net form's three layers of mask words (the formulas of the rollout suites' tests of the same name)
    per_stage_row = ns * nc * 4 + 7 * 16 if m.affine else 48
    expect = out.numel() * 4 + Hc * mf * S * B * per_stage_row
    print("%s: forward kept %.2f MB; outputs + kept per fine stage: %.2f MB" % (kind, grown / 1e6, expect / 1e6))
    assert grown <= 2 * expect, "forward kept %.1f MB (outputs + kept per fine stage: %.1f MB)" % (grown / 1e6, expect / 1e6)
    out.sum().backward()
