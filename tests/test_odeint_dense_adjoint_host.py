"""Host-side checks of ``nlbac_amd.ode_dense.odeint_dense_adjoint`` (no GPU needed): every argument ``odeint_dense``
refuses is refused with the same error type before anything touches a device, the hand-over kernel's entry point is
declared in the header and in the binding's table, and the CPU reference the GPU tests compare against
(``dense_adjoint_common``) pins itself — to the step sequences its two cases were chosen for, to the direct gradient of
the same dense solve, and to ``O.odeint_adjoint`` where the grid has two points."""
import os
import re

import pytest
import torch

import dense_adjoint_common as A
import dense_common as D
from oracle import nlbac_oracle as O

GRID = [0.0, 0.01, 0.02, 0.05, 0.3]


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


def test_odeint_dense_adjoint_refuses_foreign_modules():
    from nlbac_amd.ode_dense import odeint_dense_adjoint
    with pytest.raises(TypeError):
        odeint_dense_adjoint(torch.nn.Linear(5, 5), torch.zeros(4, 5), GRID)


@pytest.mark.parametrize("kind,width", [("affine", 5), ("concat", 12)])
def test_odeint_dense_adjoint_validates_before_touching_a_device(kind, width, monkeypatch):
    from nlbac_amd import _lib
    from nlbac_amd.ode_dense import odeint_dense_adjoint
    m = model(kind)

    def no_device(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(type(m), "refresh_device_weights", no_device)
    monkeypatch.setattr(type(m), "device_handles", no_device)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", no_device)
    y0 = torch.zeros(4, width)
    nan, inf = float("nan"), float("inf")
    bad = [
        (ValueError, dict(t=[0.0])),                                   # T < 2
        (ValueError, dict(t=[])),
        (ValueError, dict(t=torch.zeros(2, 3))),                       # not 1-D
        (ValueError, dict(t=[0.0, 0.02, 0.02, 0.05])),                 # a repeated point
        (ValueError, dict(t=[0.0, 0.05, 0.02, 0.1])),                  # not monotone
        (ValueError, dict(t=[0.1, 0.05, 0.0])),                        # decreasing: out of scope
        (ValueError, dict(t=[0.0, nan, 0.1])),
        (ValueError, dict(t=[0.0, 0.02, inf])),
        (ValueError, dict(t=torch.tensor([0.0, 1e-50], dtype=torch.float64))),     # an interval that is 0 in float32
        (TypeError, dict(t=torch.tensor([False, True]))),
        (ValueError, dict(atol=0.0)),
        (ValueError, dict(atol=-1e-7)),
        (ValueError, dict(atol=nan)),
        (ValueError, dict(rtol=0.0)),
        (ValueError, dict(rtol=inf)),
        (TypeError, dict(rtol="1e-5")),
        (TypeError, dict(atol=True)),
        (TypeError, dict(atol=torch.tensor(1e-7))),
        (NotImplementedError, dict(adjoint_params=[next(m.parameters())])),        # a subset of the parameters
        (ValueError, dict(y0=torch.zeros(4, width + 1))),
        (ValueError, dict(y0=torch.zeros(4, width - 1))),
        (ValueError, dict(y0=torch.zeros(width))),
        (ValueError, dict(y0=torch.zeros(0, width))),
        (TypeError, dict(y0=torch.zeros(4, width, dtype=torch.float64))),
        (TypeError, dict(y0=[[0.0] * width])),
        (ValueError, dict()),             # a CPU tensor: a CUDA device is required
        (ValueError, dict(adjoint_params=())),                         # (the same with no parameter adjoint)
    ]
    for exc, kw in bad:
        args = dict(y0=y0, t=GRID)
        args.update(kw)
        with pytest.raises(exc):
            odeint_dense_adjoint(m, args.pop("y0"), args.pop("t"), **args)
    with pytest.raises(TypeError):
        odeint_dense_adjoint(m, y0, GRID, method="rk4")                # the method is dopri5: no such keyword
    with pytest.raises(TypeError):
        odeint_dense_adjoint(m, y0, GRID, adjoint=True)                # the entry IS the adjoint: no such keyword


def test_the_neighbouring_entries_still_refuse_and_point_here():
    from nlbac_amd.ode_dense import odeint_dense
    from nlbac_amd.odeint import odeint_adjoint
    m = model("affine")
    with pytest.raises(NotImplementedError, match="odeint_dense_adjoint"):
        odeint_dense(m, torch.zeros(4, 5), GRID, adjoint=True)
    with pytest.raises(NotImplementedError, match="time points"):
        odeint_adjoint(m, torch.zeros(4, 5), GRID)
    assert "odeint_dense_adjoint" in odeint_adjoint.__doc__


def test_interval_lengths_are_differences_of_the_float32_entries():
    from nlbac_amd import ode_dense
    t32 = torch.tensor([0.1, 0.3, 0.6])
    want = tuple(float(t32[j]) - float(t32[j - 1]) for j in (1, 2))
    for t in ([0.1, 0.3, 0.6], t32, t32.double(), (0.1, 0.3, 0.6)):
        assert ode_dense._lengths(t) == want
    # two points: the one length IS the forward's span, so the adjoint solve runs over odeint_adjoint's dt
    assert ode_dense._lengths(t32[[0, 2]]) == ode_dense._taus(t32[[0, 2]])


def test_exports_and_header_declare_the_restart():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    assert re.search(r"#define NLBAC_ABI_VERSION 17\b", raw) and _lib.ABI_VERSION == 17
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    name = "nlbac_adj_dense_restart"
    assert name in _lib.EXPORTS
    proto = re.search(r"int %s\s*\((.*?)\);" % name, txt, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS[name]) == 10
    for arg in ("long y_ld", "long dout_ld", "const float *Zprev", "float *Z0"):
        assert arg in proto, arg


@pytest.mark.parametrize("name", A.NAMES)
def test_reference_takes_the_sequences_the_cases_were_chosen_for(name):
    """Forward: two accepted steps, none rejected, two outputs each, no output time near a step's end.  Backward without
    the parameter adjoint: the listed attempts per interval, none rejected, no error ratio within 0.25 of 1 — so that the
    device, whose ratios carry fp32 noise at the 1e-3 level, must take the same decisions."""
    c = A.case(name)
    times = D.times_of(c["t"])
    taus = [v - times[0] for v in times[1:]]
    assert all(s[2] for s in c["steps"]), c["steps"]
    assert [s[0] for s in c["steps"]] == pytest.approx(A.WANT_STEPS[name], rel=2e-3)
    assert D.outputs_per_step(c["ends"], times) == [2, 2]
    assert min(abs(e - x) for e in c["ends"] for x in taus) > 2e-3 * taus[-1]
    r = A.adjoint(name, False)
    print(name, "adjoint step logs, last interval first:", r["logs"])
    assert r["attempts"] == A.WANT_ATTEMPTS[name]
    for log in r["logs"]:
        assert all(acc for _, _, acc in log), log
        assert all(abs(ratio - 1.0) >= 0.25 for _, ratio, _ in log), log


@pytest.mark.parametrize("name", A.NAMES)
@pytest.mark.parametrize("with_params", [False, True])
def test_reference_adjoint_agrees_with_the_direct_gradient(name, with_params):
    """The continuous adjoint against back-propagation through the same dense solve: solver tolerance
    (``test_adjoint_gpu``'s dopri5 bar for T < 0.1)."""
    c = A.case(name)
    r = A.adjoint(name, with_params)
    e = A.rel_l2(r["gy0"].numpy(), c["gy0_direct"].numpy())
    print("%s (parameter adjoint %s): gy0 adjoint vs direct, rel L2 %.3g; attempts %s" % (name, with_params, e, r["attempts"]))
    assert e < 5e-3
    if with_params:
        print("%s: parameter adjoint vs direct, rel L2 %.3g" % (name, A.rel_l2(r["gp"].numpy(), c["gp_direct"].numpy())))


@pytest.mark.parametrize("name", A.NAMES)
@pytest.mark.parametrize("with_params", [False, True])
def test_two_points_are_the_oracles_odeint_adjoint(name, with_params):
    """One interval: the walk is ``O.odeint_adjoint`` itself, bit for bit.  The output gradient at t1 is zero on the
    carried columns here: ``O.odeint_adjoint`` takes those into the augmented state (where they meet the norm), the
    reference — as the device — adds them outside; with zeros there the two are the same arithmetic.  The gradient at t0
    is nonzero on every column."""
    c = A.case(name)
    ns, times = c["n_s"], D.times_of(c["t"])
    dout = c["dout"][[0, -1]].clone()
    dout[1][:, ns:] = 0
    sd = {k: torch.tensor(v, requires_grad=True) for k, v in c["W"].items()}
    node = D.CASES[name]["node"](sd)
    params = tuple(sd.values()) if with_params else ()
    yy = c["y0"].clone().requires_grad_(True)
    info = {}
    o = O.odeint_adjoint(node, yy, torch.tensor([times[0], times[-1]], dtype=torch.float64), method="dopri5", info=info,
                         adjoint_params=None if with_params else ())
    g = torch.autograd.grad((o * dout).sum(), (yy,) + params)
    with torch.no_grad():
        out, _, _ = D.dense_reference(node, c["y0"], [times[0], times[-1]])
    assert torch.equal(out, o.detach())
    gy0, th, logs = A.adjoint_backward(node, params, out, dout, [times[0], times[-1]], ns)
    assert logs == [info["adjoint_steps"]]
    assert torch.equal(gy0, g[0])
    assert len(th) == len(g) - 1 and all(torch.equal(a, b) for a, b in zip(th, g[1:]))
