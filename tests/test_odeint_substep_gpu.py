"""GPU: ``odeint_grid(..., step_size=s)`` — euler / rk4 steps of ``s`` on the solver's own fine grid, the output points
read off it by linear interpolation — against the parent path: ``odeint_grid`` on the fine grid itself (bit for bit where
the output points are fine-grid points; followed by the same interpolation as differentiable torch ops where they are
not), the chained path against the one-launch ``*_subgrid_*`` kernels, the launch counts, and ``odeint`` with
``options=dict(step_size=s)``.

Bounds.  States at an interpolated point: |out - (a0 + theta (a1 - a0))| <= 4 * 2^-24 * (|a0| + |a1|) elementwise, the
reference expression in float64 on the float32 fine states a0, a1: three fp32 roundings (the difference, the product,
the sum), each relative to a quantity no larger than |a0| + |a1| — 3 * 2^-24 at worst — and one unit of margin.
Gradients: 1e-5 relative to the reference's largest entry per tensor, the bar of ``test_one_launch_equals_chain`` for
gradients that differ in fp32 summation order only (the forward states are bitwise the same, so no ReLU mask differs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"unicycle": (3, 3, 6), "pvtol": (6, 6, 12), "cars": (12, 10)}
G2 = [0, 1 / 32, 3 / 32, 4 / 32, 8 / 32]
GRID = [0.0, 0.02, 0.05, 0.055, 0.1, 0.12]
KINDS = ["unicycle", "pvtol", "cars"]
STATE_BOUND = 4 * 2.0 ** -24
GRAD_BAR = 1e-5


def make(kind, seed=0, **kw):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(seed)
    m = NeuralODEModel(*SHAPES[kind], **kw)
    return m, m.n_s, (m.n_u if m.affine else m.n_carry)


def state(ns, nc, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, ns + nc, generator=g) * 2 - 1


def weights(T, B, width, seed=5):
    return torch.randn(T, B, width, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.fixture
def one_launch():
    from nlbac_amd import rollout as R
    old = R.ONE_LAUNCH
    yield R
    R.ONE_LAUNCH = old


def run(m, mode, y0, w, solve):
    """``solve(y)`` -> out under keep-mode ``mode`` with the loss (out * w).sum(): (out, y0.grad, parameter gradients)."""
    for p in m.parameters():
        p.requires_grad_(mode == "params")
    m.zero_grad()
    if mode == "none":
        with torch.no_grad():
            return solve(y0), None, []
    y = y0.clone().requires_grad_()
    out = solve(y)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), y.grad, [p.grad.clone() for p in m.parameters()] if mode == "params" else []


def sub_solve(m, t, method, s):
    from nlbac_amd.ode_grid import odeint_grid
    return lambda y: odeint_grid(m, y, t, method=method, step_size=s)


# ---- 1. / 6. output points that are fine-grid points: the parent's own code on the fine grid, bit for bit
def check_aligned(m, ns, nc, method, B, s, modes):
    from nlbac_amd.ode_grid import _sub_grid, odeint_grid
    taus, hs, ofs, theta = _sub_grid(G2, s)
    assert theta == (1.0,) * (len(G2) - 1)
    idx = [taus.index(v) for v in G2]
    y0 = state(ns, nc, B).cuda()
    w = weights(len(G2), B, ns + nc)
    w_fine = torch.zeros(len(taus), B, ns + nc, device="cuda")
    w_fine[idx] = w                   # the same weights at the output points, zeros at the unused fine points
    for mode in modes:
        out, gy, gp = run(m, mode, y0, w, sub_solve(m, G2, method, s))
        ref, ry, rp = run(m, mode, y0, w_fine, lambda y: odeint_grid(m, y, torch.tensor(taus, dtype=torch.float64), method=method))
        assert out.shape == (len(G2), B, ns + nc)
        assert torch.equal(out, ref[idx]), mode
        if mode != "none":
            assert torch.equal(gy[:, :ns], ry[:, :ns]), "%s: d/dx0" % mode
            assert torch.equal(gy[:, ns:], ry[:, ns:]), "%s: d/d carried columns" % mode
        assert len(gp) == len(rp)
        for (name, _), a, b in zip(m.named_parameters(), gp, rp):
            assert torch.equal(a, b), "%s: d/d%s" % (mode, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
@pytest.mark.parametrize("s", [1 / 32, 1 / 64])
def test_aligned_grid_equals_fine_grid_solve(kind, method, B, s):
    m, ns, nc = make(kind)
    check_aligned(m, ns, nc, method, B, s, ("none", "inputs", "params"))


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_aligned_grid_equals_fine_grid_solve_many_tiles(kind):
    m, ns, nc = make(kind)
    check_aligned(m, ns, nc, "rk4", 8192, 1 / 64, ("params",))


def test_aligned_grid_normalised_net():
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    g = torch.Generator().manual_seed(11)
    r = lambda n, lo, hi: (torch.rand(n, generator=g) * (hi - lo) + lo).numpy()
    torch.manual_seed(0)
    m = NeuralODEModel(8, 6, normalizer=(r(8, -0.5, 0.5), r(8, 0.5, 2.0), r(6, -0.3, 0.3), r(6, 0.5, 2.0)))
    check_aligned(m, m.n_s, m.n_carry, "rk4", 96, 1 / 64, ("params",))


# ---- 2. / 3. output points between fine-grid points
def fine_reference(m, ns, nc, t, method, s, mode, y0, w):
    """The parent's way: ``odeint_grid`` on the fine grid, then the interpolation as differentiable torch ops."""
    from nlbac_amd.ode_grid import _sub_grid, odeint_grid
    taus, hs, ofs, theta = _sub_grid(t, s)
    where = {j: i for i in range(len(hs)) for j in range(ofs[i], ofs[i + 1])}
    kept = {}

    def solve(y):
        fine = odeint_grid(m, y, torch.tensor(taus, dtype=torch.float64), method=method)
        kept["fine"] = fine.detach()
        pts = [fine[0]]
        for j in range(1, len(t)):
            a0, a1, th = fine[where[j]], fine[where[j] + 1], theta[j - 1]
            pts.append(a1 if th == 1.0 else (a0 if th == 0.0 else a0 + th * (a1 - a0)))
        return torch.stack(pts)

    res = run(m, mode, y0, w, solve)
    return res, kept["fine"], where, theta


def check_states(out, fine, where, theta, ns, tag):
    """Bitwise the fine state where theta is 0 or 1; elsewhere within STATE_BOUND of the float64 expression."""
    assert torch.equal(out[0], fine[0])
    worst = 0.0
    for j in range(1, out.shape[0]):
        a0, a1, th = fine[where[j]], fine[where[j] + 1], theta[j - 1]
        if th in (0.0, 1.0):
            assert torch.equal(out[j], a1 if th == 1.0 else a0), "%s: output %d" % (tag, j)
            continue
        assert torch.equal(out[j][:, ns:], fine[0][:, ns:]), "%s: carried columns of output %d" % (tag, j)
        a0, a1 = a0[:, :ns].double(), a1[:, :ns].double()
        err = (out[j][:, :ns].double() - (a0 + th * (a1 - a0))).abs()
        scale = a0.abs() + a1.abs()
        worst = max(worst, float((err / scale.clamp_min(1e-300)).max()))
        assert bool((err <= STATE_BOUND * scale).all()), "%s: output %d" % (tag, j)
    return worst


def rel(a, b):
    return float((a - b).abs().max()) / max(1e-30, float(b.abs().max()))


def check_grads(m, ns, got, ref, tag):
    (_, gy, gp), (_, ry, rp) = got, ref
    errs = dict(dx0=rel(gy[:, :ns], ry[:, :ns]), dcarried=rel(gy[:, ns:], ry[:, ns:]))
    for (name, _), a, b in zip(m.named_parameters(), gp, rp):
        errs[name] = rel(a, b)
    assert len(gp) == len(rp)
    return errs


def check_unaligned(m, ns, nc, method, B, s, modes, tag):
    y0 = state(ns, nc, B).cuda()
    w = weights(len(GRID), B, ns + nc)
    for mode in modes:
        got = run(m, mode, y0, w, sub_solve(m, GRID, method, s))
        ref, fine, where, theta = fine_reference(m, ns, nc, GRID, method, s, mode, y0, w)
        worst = check_states(got[0], fine, where, theta, ns, tag)
        errs = check_grads(m, ns, got, ref, tag) if mode != "none" else {}
        print("%s %s s=%g B=%d %s: states %.3g of (|a0| + |a1|) (bound %.3g)  gradients (relative to the reference's "
              "largest entry) %s" % (tag, method, s, B, mode, worst, STATE_BOUND,
                                     "  ".join("%s %.3g" % kv for kv in errs.items()) or "-"))
        for k, e in errs.items():
            assert e <= GRAD_BAR, "%s %s: d/d%s %.3g" % (tag, mode, k, e)
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
@pytest.mark.parametrize("s", [0.03, 0.2, 0.007])
def test_unaligned_grid_against_fine_grid_and_torch_interpolation(kind, method, B, s):
    m, ns, nc = make(kind)
    check_unaligned(m, ns, nc, method, B, s, ("none", "inputs", "params"), kind)


def spy(monkeypatch):
    from nlbac_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("s", [0.03, 0.2, 0.007])
def test_chained_path_and_one_launch_against_it(one_launch, monkeypatch, kind, method, s):
    from nlbac_amd.ode_grid import _sub_grid
    m, ns, nc = make(kind)
    B = 40
    one_launch.ONE_LAUNCH = True
    one = check_unaligned(m, ns, nc, method, B, s, ("params",), kind + " one launch")
    one_launch.ONE_LAUNCH = False
    calls = spy(monkeypatch)
    chained = check_unaligned(m, ns, nc, method, B, s, ("params",), kind + " chained")
    assert calls and not [n for n in calls if "_subgrid_" in n or "_grid_" in n or "_traj_" in n], calls
    # one launch against chained: the same fine states, so bitwise the same wherever no interpolation happens (each is
    # within STATE_BOUND of the float64 expression elsewhere: checked above)
    theta = _sub_grid(GRID, s)[3]
    for j in range(len(GRID)):
        if j == 0 or theta[j - 1] in (0.0, 1.0):
            assert torch.equal(one[0][j], chained[0][j]), "output %d" % j
    errs = check_grads(m, ns, one, chained, kind)
    print("%s %s s=%g one launch vs chained: %s" % (kind, method, s, "  ".join("%s %.3g" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= GRAD_BAR, "d/d%s %.3g" % (k, e)


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("s", [0.03, 0.2, 0.007])
def test_refused_net_takes_the_chained_path(monkeypatch, kind, method, s):
    from nlbac_amd import rollout as R
    m, ns, nc = make(kind, hidden_dim=160)
    assert R.ONE_LAUNCH and not R._one_launch_ok(m, method)
    calls = spy(monkeypatch)
    check_unaligned(m, ns, nc, method, 40, s, ("none", "inputs", "params"), kind + " hidden 160")
    assert calls and not [n for n in calls if "_subgrid_" in n or "_grid_" in n or "_traj_" in n], calls


# ---- 4. launch counts
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params", [False, True])
def test_sub_grid_launch_counts(one_launch, monkeypatch, kind, params):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    for p in m.parameters():
        p.requires_grad_(params)
    y0 = state(ns, nc, 96).cuda().requires_grad_()
    one_launch.ONE_LAUNCH = True
    calls = spy(monkeypatch)
    out = odeint_grid(m, y0, GRID, method="rk4", step_size=0.007)
    fam = "nlbac_node_rk" if m.affine else "nlbac_concat_rk"
    assert [n for n in calls if n.startswith(fam)] == [fam + "_subgrid_fwd"], calls
    del calls[:]
    out.sum().backward()
    assert calls == [fam + "_subgrid_bwd"] + (["nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"] if params else []), calls


# ---- 5. odeint with options=dict(step_size=s)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_odeint_with_step_size(kind, method):
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.odeint import odeint
    m, ns, nc = make(kind)
    y0 = state(ns, nc, 40).cuda()
    t = [0.01, 0.03]
    w = weights(2, 40, ns + nc)
    a = run(m, "params", y0, w, lambda y: odeint(m, y, t, method=method, options=dict(step_size=0.004)))
    b = run(m, "params", y0, w, lambda y: odeint_grid(m, y, t, method=method, step_size=0.004))
    assert a[0].shape == (2, 40, ns + nc) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    with torch.no_grad():
        assert not torch.equal(a[0][1], odeint(m, y0, t, method=method)[1])      # (five steps are not one)
        # N = 1, theta = 1: the one step of plain odeint
        assert torch.equal(odeint(m, y0, torch.tensor(t), method=method, options=dict(step_size=0.02)),
                           odeint(m, y0, torch.tensor(t), method=method))
