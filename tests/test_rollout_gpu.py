"""GPU: ``nlbac_amd.rollout.rollout`` — H env steps ahead with a new control per interval, differentiable — against the
chain of reference-shaped ``odeint`` calls (bit for bit), the CPU oracle's composition of one-interval solves (gradients),
and the one-launch trajectory kernels against the chained path (``ONE_LAUNCH`` off)."""
import numpy as np
import pytest
import torch

from oracle import nlbac_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = {"unicycle": (3, 3, 6), "pvtol": (6, 6, 12), "cars": (12, 10)}


def make(kind, seed=0):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(seed)
    m = NeuralODEModel(*SHAPES[kind])
    ns = m.n_s
    nc = m.n_u if m.affine else m.n_carry
    return m, ns, nc


def inputs(ns, nc, B, H, seed=3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, ns, generator=g) * 2 - 1
    c = torch.rand(H, B, nc, generator=g) * 2 - 1
    return x0, c


@pytest.fixture
def one_launch():
    from nlbac_amd import rollout as R
    old = R.ONE_LAUNCH
    yield R
    R.ONE_LAUNCH = old


@pytest.mark.parametrize("kind", ["unicycle", "pvtol", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4", "dopri5"])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("B", [96, 8192])
def test_rollout_equals_chained_odeint(kind, method, H, B):
    from nlbac_amd.odeint import odeint
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    x0, c = inputs(ns, nc, B, H)
    x0, c = x0.cuda(), c.cuda()
    dt = 0.02
    with torch.no_grad():
        out = rollout(m, x0, c, dt, method=method)
        assert out.shape == (H + 1, B, ns)
        assert torch.equal(out[0], x0)
        x = x0
        for k in range(H):
            x = odeint(m, torch.cat([x, c[k]], 1), torch.tensor([0.0, dt]), method=method, atol=1e-7, rtol=1e-5)[-1][:, :ns]
            assert torch.equal(out[k + 1], x), "interval %d" % k


def _oracle_chain(ref, x0, c, dt, method):
    t = torch.tensor([0.0, dt])
    xs = [x0]
    for k in range(c.shape[0]):
        xs.append(O.odeint(ref, torch.cat([xs[-1], c[k]], 1), t, method=method)[-1][:, :x0.shape[1]])
    return torch.stack(xs)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


@pytest.mark.parametrize("kind", ["unicycle", "pvtol", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4", "dopri5"])
def test_rollout_gradients_match_oracle(kind, method):
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    B, H, dt = 96, 6, 0.02
    x0, c = inputs(ns, nc, B, H)
    w = torch.randn(H + 1, B, ns, generator=torch.Generator().manual_seed(5))
    sd = {k: v.detach().clone().requires_grad_() for k, v in m.state_dict().items()}
    ref = O.AffineNode(sd, n_s=ns, n_u=nc) if m.affine else O.ConcatNode(sd)
    x0r, cr = x0.clone().requires_grad_(), c.clone().requires_grad_()
    out_r = _oracle_chain(ref, x0r, cr, dt, method)
    (out_r * w).sum().backward()
    x0d, cd = x0.cuda().requires_grad_(), c.cuda().requires_grad_()
    out_d = rollout(m, x0d, cd, dt, method=method)
    (out_d * w.cuda()).sum().backward()
    assert _rel(out_d, out_r) < 1e-4
    gref = {k: v.grad.clone() for k, v in sd.items()}
    # rows whose ORACLE gradient itself moves by more than the bar under a 3e-6 nudge of x0 sit on a ReLU kink
    x0n = (x0 + 3e-6).requires_grad_()
    cn = c.clone().requires_grad_()
    (_oracle_chain(ref, x0n, cn, dt, method) * w).sum().backward()
    scale = lambda t: max(1e-6, float(t.abs().max()))
    kink = ((x0n.grad - x0r.grad).abs().amax(1) > 1e-4 * scale(x0r.grad)) | \
           ((cn.grad - cr.grad).abs().amax((0, 2)) > 1e-4 * scale(cr.grad))
    keep = ~kink
    assert int(keep.sum()) >= B - 4, "too many rows on a kink (%d)" % int(kink.sum())
    assert float((x0d.grad.cpu()[keep] - x0r.grad[keep]).abs().max()) < 1e-4 * scale(x0r.grad), "d/dx0"
    assert float((cd.grad.cpu()[:, keep] - cr.grad[:, keep]).abs().max()) < 1e-4 * scale(cr.grad), "d/dcontrols"
    for k, p in m.named_parameters():
        a, b = p.grad.detach().cpu().double(), gref[k].double()
        if method == "dopri5":
            err = float((a - b).norm()) / max(1e-9, float(b.norm()))
            assert err < 1e-3, "d/d%s: relative error %.3g (norm)" % (k, err)
        else:
            assert _rel(a, b) < 2e-4, "d/d%s" % k


@pytest.mark.parametrize("kind", ["unicycle", "pvtol"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [96, 8192])
@pytest.mark.parametrize("params", [False, True])
def test_one_launch_equals_chain(one_launch, kind, method, B, params):
    m, ns, nc = make(kind)
    H, dt = 8, 0.02
    x0, c = inputs(ns, nc, B, H)
    w = torch.randn(H + 1, B, ns, generator=torch.Generator().manual_seed(5)).cuda()
    for p in m.parameters():
        p.requires_grad_(params)
    res = []
    for on in (True, False):
        one_launch.ONE_LAUNCH = on
        x0d, cd = x0.cuda().requires_grad_(), c.cuda().requires_grad_()
        m.zero_grad()
        out = one_launch.rollout(m, x0d, cd, dt, method=method)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        res.append((out.detach(), x0d.grad, cd.grad, [p.grad.clone() for p in m.parameters()] if params else []))
    (o1, dx1, dc1, gp1), (o0, dx0, dc0, gp0) = res
    assert torch.equal(o1, o0)
    assert torch.equal(dx1, dx0)
    assert torch.equal(dc1, dc0)
    for a, b in zip(gp1, gp0):
        assert float((a - b).norm()) <= 1e-5 * max(1e-12, float(b.norm()))


def test_input_grads_keep_no_rows():
    from nlbac_amd.rollout import rollout
    m, ns, nc = make("unicycle")
    B, H, S = 8192, 16, 4
    x0, c = inputs(ns, nc, B, H)
    x0 = x0.cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    cd = c.cuda().requires_grad_()
    rollout(m, x0, cd, 0.02, method="rk4").sum().backward()       # warm-up: caches, weight packs
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = rollout(m, x0, cd, 0.02, method="rk4")
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    expect = out.numel() * 4 + H * S * B * (ns * nc * 4 + 7 * 16)
    assert grown <= 2 * expect, "forward kept %.1f MB (outputs + G + mask words: %.1f MB)" % (grown / 1e6, expect / 1e6)
    out.sum().backward()


def test_rollout_leaves_the_agent_alone():
    from test_agent_parity_gpu import make_agent
    from nlbac_amd import synth
    from nlbac_amd.rollout import rollout
    B, hidden, seed = 128, 256, 0
    tr = synth.unicycle_transitions(4096, seed=3)
    fields = ("obs", "action", "reward", "constraint", "center", "next_center", "next_obs", "mask")
    runs = []
    for with_rollout in (False, True):
        agent, env = make_agent(B, hidden, seed, "rk4")
        rs = np.random.RandomState(5)
        rets = []
        for updates in range(2):
            idx = rs.choice(4096, B, replace=False)
            nidx = rs.choice(4096, 1024, replace=False)
            agent.set_noise(synth.normal_eps(3, B, 2, seed=updates))
            host = tuple(tr[f][idx] for f in fields)
            node = tuple(tr[f][nidx] for f in ("obs", "action", "next_obs"))
            rets.append(agent.update_from_host(host, updates, node))
            if with_rollout and updates == 0:
                m = agent.neural_ode_model
                x0 = torch.rand(64, m.n_s, device="cuda")
                cd = torch.rand(4, 64, m.n_u, device="cuda").requires_grad_()
                rollout(m, x0, cd, 0.02, method="rk4").sum().backward()
                assert cd.grad is not None and all(p.grad is not None for p in m.parameters())
                for p in m.parameters():
                    p.grad = None
        torch.cuda.synchronize()
        runs.append((agent, rets))
    (a0, r0), (a1, r1) = runs
    np.testing.assert_array_equal(np.array(r0), np.array(r1))
    for ar0, ar1 in ((a0.ar_c, a1.ar_c), (a0.ar_a, a1.ar_a), (a0.ar_n, a1.ar_n)):
        assert torch.equal(ar0.theta, ar1.theta) and torch.equal(ar0.m, ar1.m) and torch.equal(ar0.v, ar1.v)


@pytest.mark.parametrize("kind", ["unicycle", "pvtol"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_one_launch_counts(one_launch, monkeypatch, kind, method):
    from nlbac_amd import _lib
    m, ns, nc = make(kind)
    H, B = 8, 96
    x0, c = inputs(ns, nc, B, H)
    x0, cd = x0.cuda(), c.cuda().requires_grad_()
    for p in m.parameters():
        p.requires_grad_(False)
    one_launch.ONE_LAUNCH = True
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = one_launch.rollout(m, x0, cd, 0.02, method=method)
    fwd = [n for n in calls if n.startswith("nlbac_node_rk")]
    assert fwd == ["nlbac_node_rk_traj_fwd"], fwd
    del calls[:]
    out.sum().backward()
    assert calls == ["nlbac_node_rk_traj_bwd"], calls
