"""Host-side checks of ``ode_node.SolveNode`` (CPU tensors, no library): the one autograd node of every NODE solve
entry, over a toy solve written in plain torch with two inputs and two parameters —

    out = a * w + b @ v          a, b (3, 2); w (2,), v (2, 2)

— whose backward hands back (da, db, the flat parameter gradient [dw | dv]) as the real solves do.  What is checked is
the node's bookkeeping: which gradient goes to which argument, what the solve is told about who asks, when ``out`` is a
saved tensor, and the messages."""
import itertools

import pytest
import torch


class Arena:
    def __init__(self, params):
        self.offset_of, n = {}, 0
        for p in params:
            self.offset_of[id(p)] = n
            n += p.numel()


class Func:
    """What ``param_grads`` asks of a model: its parameters, and their offsets in the first handle's arena."""

    def __init__(self, w, v):
        self.params = [w, v]
        self.arena = Arena(self.params)

    def parameters(self):
        return iter(self.params)

    def device_handles(self):
        return [self]


class ToySolve:
    api = "toy_entry"

    def __init__(self, func, with_params=True, saves_out=False, keep=True):
        self.func, self.with_params, self.saves_out, self.keep, self.kept = func, with_params, saves_out, keep, None
        self.calls = []

    def forward(self, a, b):
        assert not a.requires_grad and not b.requires_grad, "the node hands over detached inputs"
        w, v = (p.detach() for p in self.func.params)
        self.kept = (a, b) if self.keep else None
        return a * w + b @ v

    def backward(self, dout, need_in, need_p, **kw):
        self.calls.append((tuple(need_in), need_p, kw))
        (a, b), (w, v) = self.kept, (p.detach() for p in self.func.params)
        flat = torch.cat([(dout * a).sum(0), (b.t() @ dout).flatten()]) if need_p else None
        return dout * w, dout @ v.t(), flat


def tensors(requires):
    g = torch.Generator().manual_seed(0)
    shapes = ((3, 2), (3, 2), (2,), (2, 2))
    return [torch.randn(*s, generator=g).requires_grad_(r) for s, r in zip(shapes, requires)]


@pytest.mark.parametrize("requires", [r for r in itertools.product([False, True], repeat=4) if any(r)])
def test_every_subset_gets_its_gradients_and_nothing_else(requires):
    from nlbac_amd.ode_node import SolveNode
    dout = torch.randn(3, 2, generator=torch.Generator().manual_seed(1))
    a, b, w, v = tensors(requires)
    solve = ToySolve(Func(w, v))
    out = SolveNode.apply(solve, 2, a, b, w, v)
    (out * dout).sum().backward()
    ra, rb, rw, rv = ref = tensors(requires)
    ((ra * rw + rb @ rv) * dout).sum().backward()
    for name, t, r, asked in zip("abwv", (a, b, w, v), ref, requires):
        assert (t.grad is not None) == asked, name
        if asked:
            assert t.grad.shape == t.shape and torch.allclose(t.grad, r.grad, rtol=1e-6, atol=1e-6), name
    (need_in, need_p, kw), = solve.calls
    assert need_in == tuple(requires[:2]) and need_p == any(requires[2:]) and kw == {}


def test_a_solve_that_does_not_differentiate_its_parameters_returns_none_for_them():
    """``odeint_adjoint(adjoint_params=())``: the parameters ask, the solve has no gradient for them."""
    from nlbac_amd.ode_node import SolveNode
    a, b, w, v = tensors((True, False, True, True))
    solve = ToySolve(Func(w, v), with_params=False)
    SolveNode.apply(solve, 2, a, b, w, v).sum().backward()
    assert a.grad is not None and b.grad is None and w.grad is None and v.grad is None
    assert solve.calls == [((True, False), False, {})]


@pytest.mark.parametrize("saves_out", [True, False])
def test_out_is_a_saved_tensor_exactly_for_a_solve_that_reads_it(saves_out):
    from nlbac_amd.ode_node import SolveNode
    a, b, w, v = tensors((True, True, True, True))
    solve = ToySolve(Func(w, v), saves_out=saves_out)
    out = SolveNode.apply(solve, 2, a, b, w, v)
    kept_out = out.detach().clone()
    SolveNode.apply(solve, 2, a, b, w, v).sum().backward()          # (untouched: the backward gets ``out`` back)
    if saves_out:
        assert set(solve.calls[-1][2]) == {"out"} and torch.equal(solve.calls[-1][2]["out"], kept_out)
    else:
        assert solve.calls[-1][2] == {}
    out.add_(1.0)
    if saves_out:
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            out.sum().backward()
    else:
        out.sum().backward()


def test_a_forward_without_gradients_has_no_backward():
    from nlbac_amd.ode_node import SolveNode
    a, b, w, v = tensors((True, True, True, True))
    out = SolveNode.apply(ToySolve(Func(w, v), keep=False), 2, a, b, w, v)
    with pytest.raises(AssertionError, match=r"toy_entry: nothing was kept for a backward \(the forward ran without gradients\)"):
        out.sum().backward()


def test_a_solve_whose_forward_kept_nothing_saves_no_out():
    from nlbac_amd.ode_node import SolveNode
    a, b, w, v = tensors((True, True, True, True))
    out = SolveNode.apply(ToySolve(Func(w, v), saves_out=True, keep=False), 2, a, b, w, v)
    assert out.grad_fn.saved_tensors == ()
