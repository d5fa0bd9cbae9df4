"""GPU: ``rollout(adjoint=True)`` / ``odeint_grid(adjoint=True)`` — the continuous adjoint on a grid, one backward launch
(``nlbac_node_adj_traj`` / ``nlbac_concat_adj_traj``) — against the autograd chain of this build's one-interval
``odeint_adjoint`` calls (bit for bit in the input gradients; ``tests/test_adjoint_gpu.py`` pins that call to the oracle),
against the chained adjoint path, against a float64 restatement of the sub-stepped rule, in chunks, and by what it keeps."""
import gc

import pytest
import torch

from oracle import nlbac_oracle as O
from common import vec_close
from test_rollout_concat_gpu import make as make_concat
from test_rollout_gpu import make as make_affine

pytestmark = pytest.mark.gpu

KINDS = ("unicycle", "pvtol", "cars", "quadrotor")
DT, STEP = 0.01, 0.004          # m = 3 fine steps per control interval, the last one cut
GRID = [0.0, 0.01, 0.013, 0.03]


def make(kind):          # (wide: SimulatedCars' net at 160 units, which the register-resident kernels refuse)
    return (make_affine if kind in ("unicycle", "pvtol") else make_concat)(kind)


def inputs(ns, nc, B, H, seed=3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, ns, generator=g) * 2 - 1
    c = torch.rand(H, B, nc, generator=g) * 2 - 1
    w = torch.randn(H + 1, B, ns, generator=g)
    return x0.cuda(), c.cuda(), w.cuda()


@pytest.fixture
def one_launch():
    from nlbac_amd import rollout as R
    old = R.ONE_LAUNCH
    yield R
    R.ONE_LAUNCH = old


@pytest.fixture
def calls(monkeypatch):
    from nlbac_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def set_mode(m, params):
    for p in m.parameters():
        p.requires_grad_(params)
        p.grad = None


def run_rollout(m, x0, c, w, params, **kw):
    from nlbac_amd.rollout import rollout
    set_mode(m, params)
    x0d, cd = x0.clone().requires_grad_(), c.clone().requires_grad_()
    out = rollout(m, x0d, cd, DT, **kw)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x0d.grad, cd.grad, [p.grad.clone() for p in m.parameters()] if params else []


def close_params(got, want, name=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.double(), b.double()
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()), "%s parameter %d: %.3g of %.3g" % (
            name, i, float((a - b).norm()), float(b.norm()))


# ---- 1. the chain of odeint_adjoint calls -------------------------------------------------------------------------------
def chain_of_odeint_adjoint(m, y0, ctrl_of, t_of, H, w, method, params):
    """The autograd chain of one-interval ``odeint_adjoint`` calls over full rows y = [x | carried], walked as autograd
    walks it — last interval first, the gradient of y_k+1 = the loss's own plus what interval k+1 sends back — but one
    call at a time (``odeint_adjoint`` keeps one solve's state per model): interval k's forward is redone from the
    stored y_k right before its backward.  ``t_of(k)``: interval k's two time points; ``ctrl_of(k)``: the carried
    columns interval k starts with, or None to carry y_k's own on.  Returns (ys, d/dy0, [d/d carried columns given per interval]); parameter gradients land in .grad."""
    from nlbac_amd.odeint import odeint_adjoint
    ns = m.n_s
    set_mode(m, params)
    ys = [y0]
    with torch.no_grad():
        for k in range(H):
            yin = ys[-1] if ctrl_of is None else torch.cat([ys[-1][:, :ns], ctrl_of(k)], 1)
            ys.append(odeint_adjoint(m, yin, torch.tensor(t_of(k)), method=method)[-1])
    carry, gcs = None, []
    for k in range(H - 1, -1, -1):
        yin = (ys[k] if ctrl_of is None else torch.cat([ys[k][:, :ns], ctrl_of(k)], 1)).clone().requires_grad_()
        y = odeint_adjoint(m, yin, torch.tensor(t_of(k)), method=method)[-1]
        y.backward(w[k + 1] if carry is None else w[k + 1] + carry)
        carry = yin.grad.clone()
        if ctrl_of is not None:
            gcs.insert(0, carry[:, ns:].clone())
            carry[:, ns:] = 0.0
    return torch.stack(ys), w[0] + carry, gcs


def rollout_chain(m, x0, c, w, method, params):
    """``chain_of_odeint_adjoint`` as a rollout: a new control per interval, the loss on the states only."""
    ns, H = m.n_s, c.shape[0]
    wy = torch.cat([w, torch.zeros(H + 1, x0.shape[0], c.shape[2], device=w.device)], 2)
    ys, gy0, gcs = chain_of_odeint_adjoint(m, torch.cat([x0, c[0]], 1), lambda k: c[k], lambda k: [0.0, DT], H, wy, method, params)
    return ys[:, :, :ns], gy0[:, :ns], torch.stack(gcs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
def test_rollout_adjoint_is_the_chain_of_odeint_adjoint(kind, method, B):
    m, ns, nc = make(kind)
    H = 3
    x0, c, w = inputs(ns, nc, B, H)
    out, gx, gc, gp = run_rollout(m, x0, c, w, True, method=method, adjoint=True)
    ref, gx_r, gc_r = rollout_chain(m, x0, c, w, method, True)
    assert torch.equal(out, ref)
    assert torch.equal(gx, gx_r), "d/dx0"
    assert torch.equal(gc, gc_r), "d/dcontrols"
    close_params(gp, [p.grad for p in m.parameters()], "rollout")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("B", [40, 96])
def test_grid_adjoint_is_the_chain_of_odeint_adjoint(kind, method, B):
    """(The loss weighs the carried columns at out[0] only: at the later grid points they are copies of y0's, and how
    autograd associates the sums of those copies' gradients is not the solver's business.)"""
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make(kind)
    g = torch.Generator().manual_seed(7)
    y0 = (torch.rand(B, ns + nc, generator=g) * 2 - 1).cuda()
    w = torch.randn(len(GRID), B, ns + nc, generator=g).cuda()
    w[1:, :, ns:] = 0.0
    set_mode(m, True)
    yd = y0.clone().requires_grad_()
    out = odeint_grid(m, yd, GRID, method=method, adjoint=True)
    (out * w).sum().backward()
    gp = [p.grad.clone() for p in m.parameters()]
    ref, gy_r, _ = chain_of_odeint_adjoint(m, y0, None, lambda k: GRID[k:k + 2], len(GRID) - 1, w, method, True)
    assert torch.equal(out.detach(), ref)
    assert torch.equal(yd.grad[:, :ns], gy_r[:, :ns]), "d/dx0"
    assert torch.equal(yd.grad[:, ns:], gy_r[:, ns:]), "d/d carried columns"
    close_params(gp, [p.grad for p in m.parameters()], "grid")


# ---- 2. one launch against the chained path ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("step", [None, STEP])
def test_one_launch_equals_chained_adjoint(one_launch, calls, kind, method, step):
    m, ns, nc = make(kind)
    B, H = 40, 3
    x0, c, w = inputs(ns, nc, B, H)
    res = []
    for on in (True, False):
        one_launch.ONE_LAUNCH = on
        del calls[:]
        res.append(run_rollout(m, x0, c, w, True, method=method, step_size=step, adjoint=True))
        traj = [n for n in calls if n.endswith("_adj_traj")]
        assert len(traj) == (1 if on else 0), calls
    (o1, gx1, gc1, gp1), (o0, gx0, gc0, gp0) = res
    assert torch.equal(o1, o0)
    assert torch.equal(gx1, gx0), "d/dx0"
    assert torch.equal(gc1, gc0), "d/dcontrols"
    close_params(gp1, gp0, "one launch vs chained")


@pytest.mark.parametrize("step", [None, STEP])
def test_grid_one_launch_equals_chained_adjoint(one_launch, step):
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make("pvtol")
    B = 40
    g = torch.Generator().manual_seed(7)
    y0 = (torch.rand(B, ns + nc, generator=g) * 2 - 1).cuda()
    w = torch.randn(len(GRID), B, ns + nc, generator=g).cuda()
    res = []
    for on in (True, False):
        one_launch.ONE_LAUNCH = on
        set_mode(m, True)
        yd = y0.clone().requires_grad_()
        out = odeint_grid(m, yd, GRID, method="rk4", step_size=step, adjoint=True)
        (out * w).sum().backward()
        res.append((out.detach(), yd.grad, [p.grad.clone() for p in m.parameters()]))
    (o1, g1, gp1), (o0, g0, gp0) = res
    assert torch.equal(o1, o0)
    assert torch.equal(g1, g0), "d/dy0"
    close_params(gp1, gp0, "grid one launch vs chained")


def test_wide_net_takes_the_chained_path(calls):
    """A 160-wide net is refused by the register-resident kernels: ``Chain`` with adjoint solvers, which IS the chain of
    ``odeint_adjoint`` calls."""
    m, ns, nc = make_concat("wide")
    x0, c, w = inputs(ns, nc, 40, 3)
    out, gx, gc, gp = run_rollout(m, x0, c, w, True, method="rk4", adjoint=True)
    assert not [n for n in calls if n.endswith("_adj_traj")] and "nlbac_concat_adj_in" in calls
    ref, gx_r, gc_r = rollout_chain(m, x0, c, w, "rk4", True)
    assert torch.equal(out, ref) and torch.equal(gx, gx_r) and torch.equal(gc, gc_r)
    close_params(gp, [p.grad for p in m.parameters()], "wide")


# ---- 3. step_size >= dt ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unicycle", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_step_size_not_below_dt_is_no_step_size(kind, method):
    m, ns, nc = make(kind)
    x0, c, w = inputs(ns, nc, 40, 3)
    a = run_rollout(m, x0, c, w, True, method=method, adjoint=True)
    for s in (DT, 1.0):
        b = run_rollout(m, x0, c, w, True, method=method, adjoint=True, step_size=s)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert all(torch.equal(p, q) for p, q in zip(a[3], b[3])), "parameter gradients"


# ---- 4. the sub-stepped sequencing against float64 -------------------------------------------------------------------
def shift_hidden_biases(m, first=4.0, growth=3.0):
    """Every hidden unit far from its kink: even units always on, odd units always off.  The first shift clears layer 0's
    own range on inputs in [-1, 1] (default initialisation: |W x + b| < (n_in + 1) / sqrt(n_in) < 4); then it grows from
    layer to layer, because so do the activations it lets through (|w h| is about half the layer below's shift)."""
    with torch.no_grad():
        for net in ([m.f_net, m.g_net] if m.affine else [m.net]):
            lin = [l for l in net if isinstance(l, torch.nn.Linear)]
            shift = first
            for l in lin[:-1]:
                l.bias[0::2] += shift
                l.bias[1::2] -= shift
                shift *= growth


class Ref64:
    """The rule of rollout(adjoint=True, step_size=s) in float64 on the CPU: forward on the fine grid from each control
    interval's lower end; backward per control interval from its upper end, y reset to the stored output, the steps of
    ``_sub_grid`` over [0, dt] in that order, z = [y | a_x | a_c] carried through, the vector-Jacobian products by
    autograd.  Records the smallest |pre-activation| met at any stage."""

    def __init__(self, m, method):
        from nlbac_amd.ode_consts import TABLEAU
        self.sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        self.ns = m.n_s
        self.node = O.AffineNode(self.sd, n_s=m.n_s, n_u=m.n_u) if m.affine else O.ConcatNode(self.sd, n_s=m.n_s, n_carry=m.n_carry)
        self.chains = [self.node.f_names, self.node.g_names] if m.affine else [self.node.names]
        self.affine = m.affine
        self.beta, self.c_sol = TABLEAU[method]["beta"], TABLEAU[method]["c_sol"]
        self.margin = float("inf")
        self.on = self.off = 0

    def watch(self, y, c):
        with torch.no_grad():
            for names in self.chains:
                x = y if self.affine else torch.cat([y, c], 1)
                for n in names[:-1]:
                    pre = O._lin(self.sd, n, x)
                    self.margin = min(self.margin, float(pre.abs().min()))
                    self.on += int((pre > 0).all(0).sum())
                    self.off += int((pre < 0).all(0).sum())
                    x = torch.relu(pre)

    def f(self, y, c):
        self.watch(y.detach(), c.detach())
        return self.node(0.0, torch.cat([y, c], 1))[:, :self.ns]

    def rk(self, G, z, h):
        ks = []
        for st in range(len(self.c_sol)):
            zs = [a + h * sum(b * k[i] for b, k in zip(self.beta[st - 1], ks) if b != 0.0) for i, a in enumerate(z)] if st else z
            ks.append(G(zs))
        return [a + h * sum(cj * k[i] for cj, k in zip(self.c_sol, ks)) for i, a in enumerate(z)]

    def solve(self, x0, c, dout, hs):
        H, ns = c.shape[0], self.ns
        params = list(self.sd.values())
        for p in params:
            p.requires_grad_(True)
        out = [x0]
        with torch.no_grad():
            for k in range(H):
                y = out[-1]
                for h in hs:
                    y, = self.rk(lambda z: [self.f(z[0], c[k])], [y], h)
                out.append(y)
        theta = [torch.zeros_like(p) for p in params]

        def G(k, z, acc, wgt):
            y, ax = z[0].detach().requires_grad_(), z[1]
            ck = c[k].detach().requires_grad_()
            F = self.f(y, ck)
            g = torch.autograd.grad(F, [y, ck] + params, grad_outputs=ax, allow_unused=True)
            for t, gt in zip(acc, g[2:]):
                if gt is not None:
                    t += wgt * gt
            return [-F.detach(), g[0], g[1]]

        ax, du = torch.zeros_like(x0), []
        for k in range(H - 1, -1, -1):
            z = [out[k + 1], dout[k + 1] + ax, torch.zeros_like(c[k])]
            for h in hs:
                # theta_bar += sum_j h c_sol[j] K_theta[j]: the stage number is the order G is called in
                stage = [0]

                def Gk(zs):
                    j = stage[0]
                    stage[0] += 1
                    return G(k, zs, theta, h * self.c_sol[j])
                z = self.rk(Gk, z, h)
            ax = z[1]
            du.insert(0, z[2])
        return torch.stack(out), dout[0] + ax, torch.stack(du), theta


# (wide: the 160-wide net, whose sub-stepped adjoint is the chained loop of one-step launches — it still answers, and right)
@pytest.mark.parametrize("kind", ["unicycle", "cars", "wide"])
def test_substepped_sequencing_against_float64(calls, kind):
    from nlbac_amd.ode_grid import _sub_grid
    m, ns, nc = make(kind)
    shift_hidden_biases(m)
    B, H = 40, 2
    x0, c, w = inputs(ns, nc, B, H)
    hs = _sub_grid(torch.tensor([0.0, DT], dtype=torch.float32), STEP)[1]
    assert len(hs) == 3 and hs[2] < hs[0]
    ref = Ref64(m, "rk4")
    out_r, gx_r, gc_r, gp_r = ref.solve(x0.cpu().double(), c.cpu().double(), w.cpu().double(), hs)
    # the condition on the test input: no pre-activation of any stage near a kink, masks not trivial
    assert ref.margin > 1e-3, "a pre-activation within 1e-3 of zero (%.3g): choose another seed" % ref.margin
    assert ref.on > 0 and ref.off > 0
    out, gx, gc, gp = run_rollout(m, x0, c, w, True, method="rk4", step_size=STEP, adjoint=True)
    assert len([n for n in calls if n.endswith("_adj_traj")]) == (0 if kind == "wide" else 1), calls
    vec_close(out.cpu().numpy(), out_r.numpy(), 1e-4, "out")
    for r in range(B):
        vec_close(gx[r].cpu().numpy(), gx_r[r].numpy(), 1e-4, "d/dx0 row %d" % r)
        vec_close(gc[:, r].cpu().numpy(), gc_r[:, r].numpy(), 1e-4, "d/dcontrols row %d" % r)
    names = [k for k, _ in m.named_parameters()]
    by_name = dict(zip(ref.sd.keys(), gp_r))
    for name, g in zip(names, gp):
        vec_close(g.cpu().numpy(), by_name[name].numpy(), 1e-4, "d/d%s" % name)


# ---- 5. chunks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pvtol", "quadrotor"])
@pytest.mark.parametrize("step", [None, STEP])
def test_chunks_change_no_bit_of_the_input_gradients(kind, step):
    m, ns, nc = make(kind)
    x0, c, w = inputs(ns, nc, 40, 3)
    whole = run_rollout(m, x0, c, w, True, method="rk4", step_size=step, adjoint=True)
    for chunk in (1, 2):
        part = run_rollout(m, x0, c, w, True, method="rk4", step_size=step, adjoint=True, adjoint_chunk=chunk)
        assert torch.equal(part[0], whole[0])
        assert torch.equal(part[1], whole[1]), "d/dx0, chunk %d" % chunk
        assert torch.equal(part[2], whole[2]), "d/dcontrols, chunk %d" % chunk
        close_params(part[3], whole[3], "chunk %d" % chunk)


def test_grid_chunks_sum_the_carried_gradient_in_the_same_order():
    from nlbac_amd.ode_grid import odeint_grid
    m, ns, nc = make("unicycle")
    g = torch.Generator().manual_seed(7)
    y0 = (torch.rand(40, ns + nc, generator=g) * 2 - 1).cuda()
    w = torch.randn(len(GRID), 40, ns + nc, generator=g).cuda()
    res = []
    for chunk in (None, 1, 2):
        set_mode(m, False)
        yd = y0.clone().requires_grad_()
        (odeint_grid(m, yd, GRID, method="rk4", step_size=STEP, adjoint=True, adjoint_chunk=chunk) * w).sum().backward()
        res.append(yd.grad)
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2])


@pytest.mark.parametrize("kind", ["unicycle", "cars"])
def test_chunk_one_is_one_launch_per_interval(calls, kind):
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    H = 3
    x0, c, w = inputs(ns, nc, 40, H)
    set_mode(m, True)
    out = rollout(m, x0, c.requires_grad_(), DT, method="rk4", adjoint=True, adjoint_chunk=1)
    del calls[:]
    (out * w).sum().backward()
    name = "nlbac_node_adj_traj" if m.affine else "nlbac_concat_adj_traj"
    assert calls == [name, "nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"] * H, calls


def test_adjoint_false_makes_the_launches_it_made(calls):
    from nlbac_amd.rollout import rollout
    m, ns, nc = make("unicycle")
    x0, c, w = inputs(ns, nc, 40, 3)
    set_mode(m, True)
    del calls[:]
    out = rollout(m, x0, c.requires_grad_(), DT, method="rk4")
    assert [n for n in calls if n.startswith("nlbac_node")] == ["nlbac_node_rk_traj_fwd"], calls
    del calls[:]
    (out * w).sum().backward()
    assert calls == ["nlbac_node_rk_traj_bwd", "nlbac_mlp_bwd_weights", "nlbac_reduce_slabs"], calls


# ---- 6. nothing is kept ------------------------------------------------------------------------------------------------
def test_forward_keeps_nothing_but_out():
    from nlbac_amd.rollout import rollout
    m, ns, nc = make("unicycle")
    B, H = 96, 8
    x0, c, _ = inputs(ns, nc, B, H)
    set_mode(m, False)
    c.requires_grad_()
    held = {}
    for key, kw in (("m1", dict(adjoint=True, step_size=DT)), ("m4", dict(adjoint=True, step_size=DT / 4)),
                    ("direct", dict(step_size=DT / 4))):
        rollout(m, x0, c, DT, method="rk4", **kw).sum().backward()       # (first-use allocations: weights, workspaces)
        c.grad = None
        # models of earlier tests are cyclic garbage (a model and the solvers cached on it refer to each other) that holds
        # device buffers: collect it now, and keep the collector from running inside the measured call
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = rollout(m, x0, c, DT, method="rk4", **kw)
            torch.cuda.synchronize()
            held[key] = torch.cuda.memory_allocated() - before
        finally:
            gc.enable()
        out_bytes = out.numel() * 4
        del out
    assert held["m1"] <= out_bytes + 64 * 1024, held
    assert held["m4"] == held["m1"], held
    assert held["direct"] > held["m4"], held


# ---- 7. dopri5 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unicycle", "cars"])
@pytest.mark.parametrize("params", [False, True])
def test_dopri5_rollout_adjoint_is_the_chain(kind, params):
    m, ns, nc = make(kind)
    B, H = 40, 2
    x0, c, w = inputs(ns, nc, B, H)
    out, gx, gc, gp = run_rollout(m, x0, c, w, params, method="dopri5", adjoint=True)
    ref, gx_r, gc_r = rollout_chain(m, x0, c, w, "dopri5", params)
    assert torch.equal(out, ref)
    assert torch.equal(gx, gx_r), "d/dx0"
    assert torch.equal(gc, gc_r), "d/dcontrols"
    if params:
        close_params(gp, [p.grad for p in m.parameters()], "dopri5")
