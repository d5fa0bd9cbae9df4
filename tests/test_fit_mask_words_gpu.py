"""GPU: the NODE fit's rows + words mode (acts_bits 2: the forward leaves the activation rows AND the ReLU mask words, the
backward gates on the words and still stores dz for the weight gradients) against the rows-only path it replaces
(``fit_words = False``, NLBAC_FIT_WORDS=0): the same gates and the same sums in the same order, so every fit — its loss,
the NODE gradient, the post-Adam parameters and Adam moments — must be bit-identical.  Covered: the headline's nets
(Unicycle), Pvtol and UnicycleBarrier at 32768 rows and at ragged row counts laid over step slots that are dirty from
fits of other sizes, the captured-graph replay of a fit, and fits that take several accepted dopri5 steps."""
import pytest
import torch

from nlbac_amd import _lib, synth
from nlbac_amd.sac_cbf_clf import _layout as SC
from test_agent_parity_gpu import make_agent

pytestmark = pytest.mark.gpu

# (row counts in order: the ragged ones follow fits of other sizes in the same 4096-row bucket, so their step slots hold
#  an earlier fit's rows and words past N; each count twice in a row: the second fit is a captured-graph replay)
SIZES = (32768, 32768, 9000, 8173, 8173)


def _fits(env_name, words, sizes, tight=False):
    agent, env = make_agent(64, 64, 0, "dopri5", env_name)
    agent.fit_solver.fit_words = words
    if tight:                     # tolerances that make the fit take several accepted steps
        agent.atol, agent.rtol = 1e-9, 1e-7
    tr = synth.transitions(env_name, max(sizes), seed=2, env=env)
    rows = agent._rows_from_host(tuple(tr[f] for f in synth.fields(env_name))).to(agent.device)
    seen = []                     # acts_bits of every nlbac_node_rk_fwd / _bwd the fits issue (captures included)
    orig = _lib.call

    def spy(name, *args):
        if name == "nlbac_node_rk_fwd" and args[20] is not None:       # (launches that keep something for a backward)
            seen.append(("fwd", args[24]))
        elif name == "nlbac_node_rk_bwd":
            seen.append(("bwd", args[18]))
        return orig(name, *args)

    out = []
    _lib.call = spy
    try:
        for N in sizes:
            agent.fit_node_rows(rows[:N])
            torch.cuda.synchronize()
            ar = agent.ar_n
            out.append(dict(N=N, steps=len(agent.fit_solver.ctx.get("steps") or []),
                            loss=agent.sc[SC.SC_NODE_LOSS:SC.SC_NODE_LOSS + 1].clone(),
                            grad=torch.cat([ar.grad_view(p).reshape(-1) for p in agent.neural_ode_model.parameters()]),
                            theta=ar.theta.clone(), m=ar.m.clone(), v=ar.v.clone()))
    finally:
        _lib.call = orig
    return out, seen


def _compare(env_name, sizes, tight=False):
    new, seen_new = _fits(env_name, True, sizes, tight)
    old, seen_old = _fits(env_name, False, sizes, tight)
    # not a vacuous pass: the new path's launches did get the rows + words mode, the old path's did not
    assert seen_new and {b for _, b in seen_new} == {2}, seen_new
    assert ("bwd", 2) in seen_new and ("fwd", 2) in seen_new
    assert seen_old and {b for _, b in seen_old} == {0}, seen_old
    for a, b in zip(new, old):
        assert a["steps"] == b["steps"], (a["N"], a["steps"], b["steps"])
        for k in ("loss", "grad", "theta", "m", "v"):
            assert torch.equal(a[k], b[k]), "%s N=%d: %s differs between the two paths" % (env_name, a["N"], k)
    return new


@pytest.mark.parametrize("env_name", ["Unicycle", "Pvtol", "UnicycleBarrier"])
def test_fit_words_match_the_rows_path(env_name):
    _compare(env_name, SIZES)


def test_fit_words_match_the_rows_path_over_several_steps():
    res = _compare("Unicycle", (32768, 8173, 8173), tight=True)
    assert all(r["steps"] >= 2 for r in res), [(r["N"], r["steps"]) for r in res]
