"""GPU: ``nlbac_amd.ode_grid.odeint_grid`` — the euler / rk4 solution of a NODE at every point of a time grid —
against the chain of ``odeint`` calls over the grid's intervals (bit for bit), the scalar-step trajectory kernels of
``rollout`` on an exactly representable uniform grid, the CPU oracle's chain of one-interval solves (gradients), and the
one-launch kernels against the chained path (``rollout.ONE_LAUNCH`` off)."""
import pytest
import torch

from oracle import nlbac_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = {"unicycle": (3, 3, 6), "pvtol": (6, 6, 12), "cars": (12, 10)}
GRID = [0.0, 0.02, 0.05, 0.055, 0.1, 0.12]
GRID7 = GRID + [0.15]
KINDS = ["unicycle", "pvtol", "cars"]


def make(kind, seed=0, **kw):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(seed)
    m = NeuralODEModel(*SHAPES[kind], **kw)
    ns = m.n_s
    nc = m.n_u if m.affine else m.n_carry
    return m, ns, nc


def state(ns, nc, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, ns + nc, generator=g) * 2 - 1


@pytest.fixture
def one_launch():
    from nlbac_amd import rollout as R
    old = R.ONE_LAUNCH
    yield R
    R.ONE_LAUNCH = old


def _chained_odeint(m, y0, t, method):
    from nlbac_amd.odeint import odeint
    ys = [y0]
    for k in range(len(t) - 1):
        ys.append(odeint(m, ys[-1], t[k:k + 2], method=method)[-1])
    return ys


# ---- 1. equals the chained odeint, bit for bit, under no_grad
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
def test_grid_equals_chained_odeint(kind, method, B):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    y0 = state(ns, nc, B).cuda()
    t = torch.tensor(GRID)
    with torch.no_grad():
        out = odeint_grid(m, y0, t, method=method)
        assert out.shape == (len(GRID), B, ns + nc)
        for k, y in enumerate(_chained_odeint(m, y0, t, method)):
            assert torch.equal(out[k], y), "grid point %d" % k


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_grid_equals_chained_odeint_many_tiles(kind):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    y0 = state(ns, nc, 8192).cuda()
    t = torch.tensor(GRID, dtype=torch.float64)
    with torch.no_grad():
        out = odeint_grid(m, y0, t, method="rk4")
        for k, y in enumerate(_chained_odeint(m, y0, t, "rk4")):
            assert torch.equal(out[k], y), "grid point %d" % k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_two_points_are_odeint_itself(kind, method):
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.odeint import odeint
    m, ns, nc = make(kind)
    y0 = state(ns, nc, 40).cuda()
    t = torch.tensor([0.01, 0.03])
    with torch.no_grad():
        assert torch.equal(odeint_grid(m, y0, t, method=method), odeint(m, y0, t, method=method))


# ---- 2. per-interval steps against the scalar-step kernels: t = k / 32 has exactly representable spacing
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_uniform_grid_equals_scalar_step_rollout(kind, method):
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    B, H = 96, 8
    for p in m.parameters():
        p.requires_grad_(False)
    y0 = state(ns, nc, B).cuda()
    w = torch.randn(H + 1, B, ns, generator=torch.Generator().manual_seed(5)).cuda()
    x0 = y0[:, :ns].clone().requires_grad_()
    c = y0[:, ns:].expand(H, B, nc).contiguous().requires_grad_()
    out_r = rollout(m, x0, c, 1 / 32, method=method)
    (out_r * w).sum().backward()
    y0g = y0.clone().requires_grad_()
    out = odeint_grid(m, y0g, [k / 32 for k in range(H + 1)], method=method)
    (out[:, :, :ns] * w).sum().backward()
    assert torch.equal(out[:, :, :ns], out_r)
    assert torch.equal(out[:, :, ns:], y0[:, ns:].expand(H + 1, B, nc))
    assert torch.equal(y0g.grad[:, :ns], x0.grad)
    ref = c.grad.sum(0)
    err = float((y0g.grad[:, ns:] - ref).abs().max()) / max(1e-12, float(ref.abs().max()))
    print("carried-column gradient vs rollout's sum over intervals: %.3g (relative to its largest entry)" % err)
    assert err <= 2e-6


# ---- 3. / 5. gradients against the oracle: O.odeint chained over the intervals
def _oracle_chain(ref, y0, t, method):
    ys = [y0]
    for k in range(len(t) - 1):
        ys.append(O.odeint(ref, ys[-1], t[k:k + 2], method=method)[-1])
    return torch.stack(ys)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def oracle_case(m, ns, nc, method, B=96, seed=3):
    """The oracle's solution and gradients on GRID7 with weights on every output point, and the rows it excuses: those
    whose ORACLE gradient itself moves by more than the bar under a 3e-6 nudge of y0 (they sit on a ReLU kink)."""
    t = torch.tensor(GRID7)
    y0 = state(ns, nc, B, seed)
    w = torch.randn(len(GRID7), B, ns + nc, generator=torch.Generator().manual_seed(5))
    sd = {k: v.detach().cpu().clone().requires_grad_() for k, v in m.state_dict().items()}
    ref = O.AffineNode(sd, n_s=ns, n_u=nc) if m.affine else O.ConcatNode(sd)
    y0r = y0.clone().requires_grad_()
    out_r = _oracle_chain(ref, y0r, t, method)
    (out_r * w).sum().backward()
    gref = {k: v.grad.clone() for k, v in sd.items()}
    y0n = (y0 + 3e-6).requires_grad_()
    (_oracle_chain(ref, y0n, t, method) * w).sum().backward()
    scale = lambda v: max(1e-6, float(v.abs().max()))
    gx, gc = y0r.grad[:, :ns], y0r.grad[:, ns:]
    kink = ((y0n.grad[:, :ns] - gx).abs().amax(1) > 1e-4 * scale(gx)) | \
           ((y0n.grad[:, ns:] - gc).abs().amax(1) > 1e-4 * scale(gc))
    return dict(t=t, y0=y0, w=w, out=out_r.detach(), gx=gx, gc=gc, gp=gref, kink=kink, scale=scale)


def check_against_oracle(m, ns, nc, method):
    from nlbac_amd.ode_grid import odeint_grid
    R = oracle_case(m, ns, nc, method)
    B = R["y0"].shape[0]
    keep = ~R["kink"]
    assert int(keep.sum()) >= B - 4, "too many rows on a kink (%d)" % int(R["kink"].sum())
    y0d = R["y0"].cuda().requires_grad_()
    out_d = odeint_grid(m, y0d, R["t"], method=method)
    (out_d * R["w"].cuda()).sum().backward()
    scale = R["scale"]
    g = y0d.grad.cpu()
    errs = dict(states=_rel(out_d, R["out"]),
                dx0=float((g[keep, :ns] - R["gx"][keep]).abs().max()) / scale(R["gx"]),
                dcarried=float((g[keep, ns:] - R["gc"][keep]).abs().max()) / scale(R["gc"]))
    perr = {k: _rel(p.grad, R["gp"][k]) for k, p in m.named_parameters()}
    print("vs oracle: %s  d/dparams max %.3g  rows excused %d" % (
        "  ".join("%s %.3g" % kv for kv in errs.items()), max(perr.values()), int(R["kink"].sum())))
    assert errs["states"] < 1e-4
    assert errs["dx0"] < 1e-4, "d/dx0"
    assert errs["dcarried"] < 1e-4, "d/d carried columns"
    for k, e in perr.items():
        assert e < 2e-4, "d/d%s" % k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_grid_gradients_match_oracle(kind, method):
    m, ns, nc = make(kind)
    check_against_oracle(m, ns, nc, method)


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_refused_net_takes_the_chained_path(monkeypatch, kind, method):
    from nlbac_amd import _lib
    from nlbac_amd import rollout as R
    m, ns, nc = make(kind, hidden_dim=160)
    assert R.ONE_LAUNCH and not R._one_launch_ok(m, method)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    check_against_oracle(m, ns, nc, method)
    assert calls and not [n for n in calls if "_grid_" in n or "_traj_" in n], calls


# ---- 4. one launch against the chained path, in the three keep-modes
def _solve(m, y0, t, method, mode, w):
    from nlbac_amd.ode_grid import odeint_grid
    for p in m.parameters():
        p.requires_grad_(mode == "params")
    m.zero_grad()
    if mode == "none":
        with torch.no_grad():
            return odeint_grid(m, y0, t, method=method), None, []
    y = y0.clone().requires_grad_()
    out = odeint_grid(m, y, t, method=method)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), y.grad, [p.grad.clone() for p in m.parameters()] if mode == "params" else []


# (every method and keep-mode at three tiles; the large batch once per kind: rk4 with parameter gradients)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method,mode,B", [(me, mo, 96) for me in ("euler", "rk4") for mo in ("none", "inputs", "params")]
                         + [("rk4", "params", 8192)])
def test_one_launch_equals_chain(one_launch, kind, method, mode, B):
    m, ns, nc = make(kind)
    y0 = state(ns, nc, B).cuda()
    w = torch.randn(len(GRID), B, ns + nc, generator=torch.Generator().manual_seed(5)).cuda()
    res = []
    for on in (True, False):
        one_launch.ONE_LAUNCH = on
        res.append(_solve(m, y0, GRID, method, mode, w))
    (o1, g1, gp1), (o0, g0, gp0) = res
    assert torch.equal(o1, o0)
    if mode != "none":
        assert torch.equal(g1[:, :ns], g0[:, :ns]), "d/dx0"
        assert torch.equal(g1[:, ns:], g0[:, ns:]), "d/d carried columns"
    for a, b in zip(gp1, gp0):
        assert float((a - b).norm()) <= 1e-5 * max(1e-12, float(b.norm()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params", [False, True])
def test_one_launch_counts(one_launch, monkeypatch, kind, params):
    from nlbac_amd import _lib
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    for p in m.parameters():
        p.requires_grad_(params)
    y0 = state(ns, nc, 96).cuda().requires_grad_()
    one_launch.ONE_LAUNCH = True
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = odeint_grid(m, y0, GRID, method="rk4")
    fam = "nlbac_node_rk" if m.affine else "nlbac_concat_rk"
    assert [n for n in calls if n.startswith(fam)] == [fam + "_grid_fwd"], calls
    del calls[:]
    out.sum().backward()
    assert calls == [fam + "_grid_bwd"] + (["nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"] if params else []), calls


# ---- 6. repeated solves and lifetime
@pytest.mark.parametrize("kind", ["unicycle", "cars"])
@pytest.mark.parametrize("on", [True, False])
def test_solves_of_different_length_on_one_model(one_launch, kind, on):
    from nlbac_amd.ode_grid import odeint_grid
    one_launch.ONE_LAUNCH = on
    grids = (GRID, GRID[:4])

    def grads(m, y0, t):
        m.zero_grad()
        y = y0.clone().requires_grad_()
        odeint_grid(m, y, t, method="rk4").sum().backward()
        return [y.grad] + [p.grad.clone() for p in m.parameters()]

    m, ns, nc = make(kind)
    y0 = state(ns, nc, 96).cuda()
    together = [grads(m, y0, t) for t in grids]
    for t, got in zip(grids, together):
        alone = grads(make(kind)[0], y0, t)
        assert all(torch.equal(a, b) for a, b in zip(got, alone)), "T = %d" % len(t)


def test_chained_backward_after_a_later_solve_is_refused(one_launch):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make("unicycle")
    y0 = state(ns, nc, 96).cuda().requires_grad_()
    one_launch.ONE_LAUNCH = False
    first = odeint_grid(m, y0, GRID, method="rk4")
    second = odeint_grid(m, y0, GRID, method="rk4")
    with pytest.raises(AssertionError, match="backward must run before the next"):
        first.sum().backward()
    second.sum().backward()


def test_grid_solvers_are_kept_apart(one_launch):
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.odeint import odeint
    from nlbac_amd.rollout import rollout
    m, ns, nc = make("unicycle")
    one_launch.ONE_LAUNCH = False
    y0 = state(ns, nc, 96).cuda().requires_grad_()
    x0 = y0.detach()[:, :ns].clone().requires_grad_()
    a = odeint(m, y0, torch.tensor([0.0, 0.02]), method="rk4")
    b = rollout(m, x0, y0.detach()[:, ns:].expand(5, 96, nc).contiguous(), 0.02, method="rk4")
    odeint_grid(m, y0, GRID, method="rk4").sum().backward()        # neither odeint's nor rollout's solvers are touched
    a.sum().backward()
    b.sum().backward()
    assert set(m.__dict__["_odeint_grid_solvers"]) == {"params"} and len(m.__dict__["_odeint_grid_solvers"]["params"]) == 5
