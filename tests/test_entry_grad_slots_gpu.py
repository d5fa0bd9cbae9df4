"""GPU: where each gradient of a NODE solve entry lands.  Every entry is one autograd node over ``(inputs..., *params)``;
which of its backward's results goes to which argument is bookkeeping no value test sees as long as everything asks
for a gradient.  Here each entry is called three times on the same seeded inputs, with ``out.sum().backward()``:

  A  everything requires a gradient;
  B  only the first parameter of ``func.parameters()`` does;
  C  only the tensor inputs do.

(i) ``.grad`` is None exactly where no gradient was asked and has the argument's shape elsewhere; (ii) B's gradient of
that first parameter is ``torch.equal`` to A's — both keep activation rows (keep mode "params") and run the same
launches, so a slot that is off by one shows as a None, a wrong shape or another tensor's values.

33 rows (one full 32-row tile and a ragged row), H = 2 control intervals or three time points, the control-affine
``NeuralODEModel(3, 3, 6)`` and, where the entry serves it, the single-net ``NeuralODEModel(12, 10)``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, H, DT = 33, 2, 0.02
T2, T3 = [0.0, 0.02], [0.0, 0.02, 0.05]


def _entries():
    from nlbac_amd.ode_dense import odeint_dense, odeint_dense_adjoint
    from nlbac_amd.ode_grid import odeint_grid
    from nlbac_amd.odeint import odeint, odeint_adjoint
    from nlbac_amd.rollout import rollout
    both, affine = ("affine", "concat"), ("affine",)
    # name: (the forms it serves, its inputs' layout, the call)
    return {
        "odeint": (both, "packed", lambda m, y0: odeint(m, y0, torch.tensor(T2), method="dopri5")),
        "odeint_adjoint": (both, "packed", lambda m, y0: odeint_adjoint(m, y0, torch.tensor(T2), method="dopri5")),
        "rollout rk4": (both, "rollout", lambda m, x0, u: rollout(m, x0, u, DT, method="rk4")),
        "rollout rk4 step_size": (both, "rollout", lambda m, x0, u: rollout(m, x0, u, DT, method="rk4", step_size=0.008)),
        "rollout rk4 adjoint": (both, "rollout", lambda m, x0, u: rollout(m, x0, u, DT, method="rk4", adjoint=True)),
        "rollout dopri5 tile": (affine, "rollout", lambda m, x0, u: rollout(m, x0, u, DT, method="dopri5",
                                                                             step_control="tile")),
        "odeint_grid rk4": (both, "packed", lambda m, y0: odeint_grid(m, y0, T3, method="rk4")),
        "odeint_grid rk4 adjoint": (both, "packed", lambda m, y0: odeint_grid(m, y0, T3, method="rk4", adjoint=True)),
        "odeint_dense batch": (both, "packed", lambda m, y0: odeint_dense(m, y0, T3, step_control="batch")),
        "odeint_dense tile": (affine, "packed", lambda m, y0: odeint_dense(m, y0, T3, step_control="tile")),
        "odeint_dense_adjoint": (both, "packed", lambda m, y0: odeint_dense_adjoint(m, y0, T3)),
    }


CASES = [("odeint", "affine"), ("odeint", "concat"), ("odeint_adjoint", "affine"), ("odeint_adjoint", "concat"),
         ("rollout rk4", "affine"), ("rollout rk4", "concat"), ("rollout rk4 step_size", "affine"),
         ("rollout rk4 step_size", "concat"), ("rollout rk4 adjoint", "affine"), ("rollout rk4 adjoint", "concat"),
         ("rollout dopri5 tile", "affine"), ("odeint_grid rk4", "affine"), ("odeint_grid rk4", "concat"),
         ("odeint_grid rk4 adjoint", "affine"), ("odeint_grid rk4 adjoint", "concat"), ("odeint_dense batch", "affine"),
         ("odeint_dense batch", "concat"), ("odeint_dense tile", "affine"), ("odeint_dense_adjoint", "affine"),
         ("odeint_dense_adjoint", "concat")]


@functools.lru_cache(maxsize=None)
def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    torch.manual_seed(0)
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


def inputs_of(m, layout):
    ns, nc = m.n_s, (m.n_u if m.affine else m.n_carry)
    g = torch.Generator().manual_seed(7)
    x0, u = torch.rand(ROWS, ns, generator=g) * 2 - 1, torch.rand(H, ROWS, nc, generator=g) * 2 - 1
    return [torch.cat([x0, u[0]], 1).cuda()] if layout == "packed" else [x0.cuda(), u.cuda()]


def grads(call, m, layout, want_inputs, want_params):
    """One forward and ``out.sum().backward()``; returns the ``.grad`` of the inputs and of the parameters."""
    params = list(m.parameters())
    for p, want in zip(params, want_params):
        p.requires_grad_(want)
        p.grad = None
    inputs = [t.requires_grad_(want_inputs) for t in inputs_of(m, layout)]
    call(m, *inputs).sum().backward()
    torch.cuda.synchronize()
    got = [t.grad for t in inputs], [None if p.grad is None else p.grad.clone() for p in params]
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    return inputs, params, got


@pytest.mark.parametrize("entry,kind", CASES)
def test_every_gradient_lands_in_its_own_slot(entry, kind):
    kinds, layout, call = _entries()[entry]
    assert kind in kinds
    m = model(kind)
    n_p = len(list(m.parameters()))
    assert n_p >= 2
    first = [True] + [False] * (n_p - 1)
    seen = {}
    for label, want_inputs, want_params in (("A", True, [True] * n_p), ("B", False, first), ("C", True, [False] * n_p)):
        inputs, params, (gin, gp) = grads(call, m, layout, want_inputs, want_params)
        for i, (t, g) in enumerate(zip(inputs, gin)):
            assert (g is not None) == want_inputs, "%s, call %s: input %d" % (entry, label, i)
            assert g is None or (g.shape == t.shape and g.device == t.device), "%s, call %s: input %d" % (entry, label, i)
        for i, (p, g, want) in enumerate(zip(params, gp, want_params)):
            assert (g is not None) == want, "%s, call %s: parameter %d" % (entry, label, i)
            assert g is None or g.shape == p.shape, "%s, call %s: parameter %d" % (entry, label, i)
        seen[label] = gp
    assert bool(seen["A"][0].abs().max() > 0), "%s: the first parameter's gradient is all zero" % entry
    assert torch.equal(seen["B"][0], seen["A"][0]), "%s: d/d(first parameter), only it asked against everything asked" % entry
