"""GPU: NODE validation — ``nlbac_traj_err_stats`` against a float64 numpy restatement of its definition (every shape
class of the thread mapping, masks, determinism, NaN propagation), ``node_fit.validate_rollout`` against ``rollout`` and
the float64 evaluation of the report's definitions, ``SAC_CBF_CLF.validate_node`` against the same reference on windows
of a device replay — and that it leaves every piece of training state as found — and the three drivers with
``node_validate_every`` on and off from the same seeds, bit for bit.

Tolerances.  ``nvalid`` and ``max`` are exact.  The four sums: every term is exact in float64 up to one rounding, and
the sum of m <= 1025 non-negative terms in any order differs from numpy's by at most about m 2^-53 = 1.2e-13 relative:
1e-12 per entry.  ``mse`` against ``traj_mse``: that kernel sums float32 in blocks of <= 1024 elements and then <= 256
partials, about 1.3k 2^-24 = 8e-5 relative: 1e-4."""
import random
import types

import numpy as np
import pytest
import torch

from fit_windows_common import episode_obs
from test_agent_parity_gpu import make_agent
from test_rollout_gpu import inputs, make

pytestmark = pytest.mark.gpu

GAMMA_B = {"Unicycle": 50.0, "SimulatedCars": 0.5, "Pvtol": 0.8}
QUIET = lambda *a: None


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def stats_ref(pred, target, x0, valid):
    """The definition in float64 numpy: (stats (5, H, n_s), nvalid)."""
    p, t, x = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (pred, target, x0))
    v = np.ones(p.shape[1], dtype=bool) if valid is None else np.asarray(valid) != 0
    e, t_v, m = (p - t)[:, v], t[:, v], (x[None] - t)[:, v]
    mx = np.abs(e).max(1) if v.any() else np.zeros((p.shape[0], p.shape[2]))
    return np.stack([(e * e).sum(1), np.abs(e).sum(1), mx, (m * m).sum(1), (t_v * t_v).sum(1)]), int(v.sum())


def mask_of(kind, n, seed):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(n)
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.6).float()


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    assert (err <= 1e-12 * np.abs(ref)).all(), "%s: relative error %.3g" % (what, float((err / np.maximum(np.abs(ref), 1e-300)).max()))


@pytest.mark.parametrize("n_s", [1, 3, 6, 10, 16])
@pytest.mark.parametrize("mask", ["none", "random", "zero"])
def test_kernel_against_float64_numpy(n_s, mask):
    from nlbac_amd.node_fit import traj_error_stats
    worst = 0.0
    for n in (1, 255, 256, 257, 1025):
        for H in (1, 2, 7):
            g = torch.Generator().manual_seed(1000 * n_s + 10 * n + H)
            pred, target, x0 = torch.randn(H, n, n_s, generator=g), torch.randn(H, n, n_s, generator=g), torch.randn(n, n_s, generator=g)
            valid = mask_of(mask, n, n + H)
            ref, nv_ref = stats_ref(pred, target, x0, valid)
            dv = None if valid is None else valid.cuda()
            stats, nvalid = traj_error_stats(pred.cuda(), target.cuda(), x0.cuda(), dv)
            again, nagain = traj_error_stats(pred.cuda(), target.cuda(), x0.cuda(), dv)
            assert stats.dtype == torch.float64 and stats.shape == (5, H, n_s) and nvalid.dtype == torch.int64
            assert torch.equal(stats, again) and torch.equal(nvalid, nagain), "two calls differ"
            got = stats.cpu().numpy()
            assert int(nvalid) == nv_ref, (n, H)
            assert (got[2] == ref[2]).all(), "max |e| is exact (n %d H %d)" % (n, H)
            for p in (0, 1, 3, 4):
                close(got[p], ref[p], "plane %d, n %d H %d" % (p, n, H))
                worst = max(worst, float((np.abs(got[p] - ref[p]) / np.maximum(np.abs(ref[p]), 1e-300)).max()))
            if mask == "zero":
                assert (got == 0.0).all() and nv_ref == 0
    print("n_s %d mask %s: largest relative difference of a sum %.3g" % (n_s, mask, worst))


@pytest.mark.parametrize("n,H,n_s", [(257, 2, 3), (1025, 7, 16), (1025, 2, 10), (1, 1, 1)])
def test_kernel_nan_propagation(n, H, n_s):
    from nlbac_amd.node_fit import traj_error_stats
    g = torch.Generator().manual_seed(n + H + n_s)
    pred, target, x0 = torch.randn(H, n, n_s, generator=g), torch.randn(H, n, n_s, generator=g), torch.randn(n, n_s, generator=g)
    valid = torch.ones(n)
    if n > 1:
        valid[torch.rand(n, generator=g) < 0.4] = 0.0
        valid[n - 1], valid[n // 2] = 1.0, 0.0
    i_on, i_off = n - 1, n // 2
    k, c = H - 1, n_s // 2
    base, nv = traj_error_stats(pred.cuda(), target.cuda(), x0.cuda(), valid.cuda())
    for bad in (float("nan"), float("inf")):
        p = pred.clone()
        p[k, i_on, c] = bad
        stats, nv2 = traj_error_stats(p.cuda(), target.cuda(), x0.cuda(), valid.cuda())
        hit = torch.zeros(5, H, n_s, dtype=torch.bool)
        hit[:3, k, c] = True
        assert not bool(torch.isfinite(stats.cpu()[hit]).any()), "a %r error stayed finite" % bad
        assert torch.equal(stats.cpu()[~hit], base.cpu()[~hit]) and int(nv2) == int(nv)
        if n > 1:                                  # the same value in an invalid window changes nothing
            p = pred.clone()
            p[k, i_off, c] = bad
            stats, _ = traj_error_stats(p.cuda(), target.cuda(), x0.cuda(), valid.cuda())
            assert torch.equal(stats, base)


# ---------------------------------------------------------------------------------------------------------------------
# validate_rollout
# ---------------------------------------------------------------------------------------------------------------------
def report_ref(pred, target, x0, valid):
    """The report's definitions in float64 torch."""
    p, t, x = pred.detach().cpu().double(), target.detach().cpu().double(), x0.detach().cpu().double()
    v = torch.ones(p.shape[1], dtype=torch.bool) if valid is None else valid.detach().cpu() != 0
    V, (H, _, n_s) = int(v.sum()), p.shape
    e, t_v, m = (p - t)[:, v], t[:, v], (x[None] - t)[:, v]
    sse, base, tss = (e * e).sum(1), (m * m).sum(1), (t_v * t_v).sum(1)
    return dict(windows_valid=V, rmse=(sse / V).sqrt(), mae=e.abs().sum(1) / V, max_abs=e.abs().amax(1),
                skill=1.0 - sse / base, nrmse=(sse / tss).sqrt(), rmse_step=(sse.sum(1) / (V * n_s)).sqrt(),
                mse=float(sse.sum() / (V * H * n_s)))


def check_report(rep, ref):
    """1e-12 relative for every quotient and root of the sums.  ``skill = 1 - r`` with r = sse / base: r carries the
    sums' 1e-12 and the subtraction adds one rounding, so skill is held to 1e-12 of the larger of itself and r — for
    a model no better than persistence (r near 1, skill near 0) a bar relative to skill alone would ask for more digits
    than r has."""
    assert rep["windows_valid"] == ref["windows_valid"]
    assert torch.equal(rep["max_abs"], ref["max_abs"])
    for key in ("rmse", "mae", "nrmse", "rmse_step"):
        assert rep[key].shape == ref[key].shape and rep[key].dtype == torch.float64, key
        close(rep[key].numpy(), ref[key].numpy(), key)
    got, want = rep["skill"].numpy(), ref["skill"].numpy()
    assert got.shape == want.shape and rep["skill"].dtype == torch.float64
    err, bar = np.abs(got - want), 1e-12 * np.maximum(np.abs(want), np.abs(1.0 - want))
    assert (err <= bar).all(), "skill: error %.3g against the bar %.3g" % (float(err.max()), float(bar.min()))
    close(rep["mse"], ref["mse"], "mse")


@pytest.mark.parametrize("kind", ["unicycle", "pvtol", "cars"])
@pytest.mark.parametrize("method", ["euler", "rk4", "dopri5"])
def test_validate_rollout(kind, method, monkeypatch):
    from nlbac_amd import node_fit
    from nlbac_amd.rollout import rollout
    m, ns, nc = make(kind)
    B, H, dt = 80, 3, 0.02
    x0, c = inputs(ns, nc, B, H)
    target = x0[None] + 0.1 * torch.randn(H, B, ns, generator=torch.Generator().manual_seed(5))
    states = torch.cat([x0[None], target]).cuda()
    valid = (torch.arange(B) % 5 != 0).float().cuda()
    seen = []
    real = node_fit.traj_error_stats
    monkeypatch.setattr(node_fit, "traj_error_stats", lambda p, *a: (seen.append(p.clone()), real(p, *a))[1])
    before = [p.detach().clone() for p in m.parameters()]
    for v in (valid, None):
        rep = node_fit.validate_rollout(m, states, c.cuda(), method, dt, valid=v)
        with torch.no_grad():
            out = rollout(m, states[0], c.cuda(), dt, method=method)
        assert torch.equal(seen[-1], out[1:]), "the predictions are not rollout's"
        check_report(rep, report_ref(out[1:], states[1:], states[0], v))
        loss = float(node_fit.traj_mse(out[1:], states[1:], v))
        assert abs(rep["mse"] - loss) <= 1e-4 * abs(loss), (rep["mse"], loss)
        assert "accepted_max" not in rep
    assert all(torch.equal(p.detach().cpu(), q.cpu()) and p.grad is None for p, q in zip(m.parameters(), before))
    # host inputs are taken as train_rollout_step takes them
    rep2 = node_fit.validate_rollout(m, states.cpu().numpy(), c.numpy(), method, dt)
    assert rep2["mse"] == rep["mse"] and torch.equal(rep2["rmse"], rep["rmse"])


def test_validate_rollout_tile_reports_the_steps():
    from nlbac_amd import node_fit
    from nlbac_amd.rollout import rollout
    from test_rollout_tile_gpu import DT, H, scaled
    m, ns, nc, x0, c, _ = scaled("pvtol")
    target = x0[None] + 0.1 * torch.randn(H, x0.shape[0], ns, generator=torch.Generator().manual_seed(6))
    states = torch.cat([x0[None], target]).cuda()
    rep = node_fit.validate_rollout(m, states, c.cuda(), "dopri5", DT, step_control="tile")
    info = {}
    with torch.no_grad():
        out = rollout(m, states[0], c.cuda(), DT, method="dopri5", step_control="tile", info=info)
    acc, att = info["accepted"].cpu().double(), info["attempts"].cpu().double()
    assert torch.equal(rep["accepted_max"], acc.amax(0)) and torch.equal(rep["attempts_max"], att.amax(0))
    close(rep["accepted_mean"].numpy(), acc.mean(0).numpy(), "accepted_mean")      # (a mean of three small integers)
    close(rep["attempts_mean"].numpy(), att.mean(0).numpy(), "attempts_mean")
    assert rep["accepted_max"].shape == (H,) and float(rep["accepted_max"].max()) > 3       # (the stiff tile takes more)
    check_report(rep, report_ref(out[1:], states[1:], states[0], None))
    mc, nsc, ncc = make("cars")
    with pytest.raises(NotImplementedError):            # rollout's own refusal: the single-net form has no tile kernels
        node_fit.validate_rollout(mc, torch.zeros(3, 8, nsc), torch.zeros(2, 8, ncc), "dopri5", 0.02, step_control="tile")


# ---------------------------------------------------------------------------------------------------------------------
# the agent
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = {1: (37, 52, 41, 60, 45, 55, 38, 49, 58, 43, 61, 61), 4: (37, 52, 41, 20)}       # 600 pushes either way


def replay_of(agent, stride, cap=1024, seed=0, **kw):
    """A device replay of 600 rows: ``stride`` interleaved lanes of episodes (observations chained inside an episode,
    noise in every other column)."""
    from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory
    lay = agent.lay
    obs, nobs = episode_obs(LENGTHS[stride], lay.obs_dim, stride)
    rows = torch.randn(len(obs), lay.LD, generator=torch.Generator().manual_seed(seed))
    scale = 0.01                                       # (the counter-fed observations, brought to the size of real ones)
    rows[:, lay.obs:lay.obs + lay.obs_dim] = torch.from_numpy(obs) * scale
    rows[:, lay.nobs:lay.nobs + lay.obs_dim] = torch.from_numpy(nobs) * scale
    mem = DeviceReplayMemory(cap, 5, agent, **kw)
    mem.push_rows(rows)
    assert len(mem) == 600
    return mem


def arenas_of(agent):
    out = []
    for a in agent.arenas:
        out += [a.theta.clone(), a.m.clone(), a.v.clone()] + ([a.target.clone()] if a.target is not None else [])
    return out


def snapshot(agent, mem):
    return dict(sc=agent.sc.clone(), arenas=arenas_of(agent), draws=mem._draws,
                counts=getattr(mem, "window_counts", None), py=random.getstate(), np=np.random.get_state(),
                cpu=torch.get_rng_state(), cuda=torch.cuda.get_rng_state(), fill=list(agent._fill),
                fit_ws=(tuple(agent._fit_ws), tuple(agent._fit_win_ws)))


def same_state(a, b):
    assert torch.equal(a["sc"], b["sc"]), "the scalars block moved"
    assert len(a["arenas"]) == len(b["arenas"]) and all(torch.equal(x, y) for x, y in zip(a["arenas"], b["arenas"]))
    assert a["draws"] == b["draws"] and a["counts"] is b["counts"]
    assert a["py"] == b["py"]
    assert all(np.array_equal(x, y) for x, y in zip(a["np"], b["np"]))
    assert torch.equal(a["cpu"], b["cpu"]) and torch.equal(a["cuda"], b["cuda"])
    assert a["fill"] == b["fill"] and a["fit_ws"] == b["fit_ws"]


def agent_ref(agent, env, mem, idx, H, stride):
    """The float64 statistics from ``sample_windows(idx=...)`` and ``rollout``."""
    from nlbac_amd.rollout import rollout
    task, N = agent.task, len(idx)
    rows, valid = mem.sample_windows(N, H, stride, idx=idx)
    p_obs, obs_ld, ctl, p_nobs, nobs_ld, _ = task.fit_inputs(rows.view(H * N, -1))
    x0, target = task.z(N, task.n_s), task.z(H, N, task.n_s)
    task.state_rows(p_obs, obs_ld, N, x0)
    task.state_rows(p_nobs, nobs_ld, H * N, target)
    with torch.no_grad():
        out = rollout(agent.neural_ode_model, x0, ctl.reshape(H, N, -1).contiguous(), float(env.dt), method=agent.solver,
                      atol=agent.atol, rtol=agent.rtol)
    return stats_ref(out[1:].cpu().numpy(), target.cpu().numpy(), x0.cpu().numpy(), valid.cpu().numpy())


@pytest.mark.parametrize("env_name,stride,solver", [("Unicycle", 1, "rk4"), ("Unicycle", 4, "rk4"), ("Unicycle", 1, "dopri5"),
                                                    ("SimulatedCars", 1, "rk4"), ("SimulatedCars", 4, "rk4")])
def test_agent_validate_node(env_name, stride, solver):
    from nlbac_amd.node_fit import error_report
    from nlbac_amd.sac_cbf_clf.sac_cbf_clf import SAC_CBF_CLF
    agent, env = make_agent(64, 64, 0, solver, env_name, GAMMA_B[env_name])
    mem = replay_of(agent, stride)
    H, N = 3, 300
    idx = torch.randint(0, len(mem), (N,), generator=torch.Generator().manual_seed(9))
    before = snapshot(agent, mem)
    assert before["counts"] is None                    # (no window was ever drawn from this replay)
    stats, nvalid = agent.validate_node(mem, N, horizon=H, stride=stride, idx=idx)
    torch.cuda.synchronize()
    same_state(before, snapshot(agent, mem))
    assert not hasattr(mem, "window_counts")
    ref, nv_ref = agent_ref(agent, env, mem, idx, H, stride)
    got = stats.cpu().numpy()
    assert stats.shape == (5, H, agent.task.n_s) and int(nvalid) == nv_ref and 0 < nv_ref < N
    assert (got[2] == ref[2]).all()
    for p in (0, 1, 3, 4):
        close(got[p], ref[p], "plane %d" % p)
    rep = error_report(stats.cpu(), int(nvalid))
    assert rep["rmse"].shape == (H, agent.task.n_s) and bool(torch.isfinite(rep["rmse"]).all())
    # a replay that has drawn windows keeps its counts; the private generator: args.seed and the tag, kept on the agent
    before = snapshot(agent, mem)
    assert before["counts"] is not None
    g = torch.Generator().manual_seed((0 * 0x9E3779B97F4A7C15 + SAC_CBF_CLF.VALIDATE_SEED_TAG) & 0x7FFFFFFFFFFFFFFF)
    firsts = [torch.randint(0, len(mem), (N,), generator=g) for _ in range(2)]
    for k in range(2):
        stats, nvalid = agent.validate_node(mem, N, horizon=H, stride=stride)
        ref_s, ref_n = agent.validate_node(mem, N, horizon=H, stride=stride, idx=firsts[k])
        assert torch.equal(stats, ref_s) and torch.equal(nvalid, ref_n)
    mine = torch.Generator().manual_seed(3)
    stats, _ = agent.validate_node(mem, N, horizon=H, stride=stride, generator=mine)
    ref_s, _ = agent.validate_node(mem, N, horizon=H, stride=stride,
                                   idx=torch.randint(0, len(mem), (N,), generator=torch.Generator().manual_seed(3)))
    assert torch.equal(stats, ref_s)
    torch.cuda.synchronize()
    same_state(before, snapshot(agent, mem))
    assert len(agent._val_ws) == 1
    # defaults: the agent's node_horizon and node_stride
    agent.node_horizon, agent.node_stride = 2, stride
    stats, _ = agent.validate_node(mem, 50)
    assert stats.shape == (5, 2, agent.task.n_s)
    agent.validate_node(mem, 70, horizon=1)
    assert len(agent._val_ws) == 2                      # (bounded at two shapes)


def test_agent_validate_node_short_replay_and_host_replay():
    from nlbac_amd import synth
    from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory, ReplayMemory
    agent, env = make_agent(64, 64, 0, "rk4", "Unicycle", GAMMA_B["Unicycle"])
    mem = DeviceReplayMemory(64, 5, agent)
    mem.push_rows(torch.randn(2, agent.lay.LD))
    assert agent.validate_node(mem, 8, horizon=3) is None
    assert agent.validate_node(mem, 8, horizon=2, stride=2) is None
    assert agent.validate_node(mem, 8, horizon=2, stride=1) is not None
    with pytest.raises(ValueError):
        agent.validate_node_windows(torch.zeros(3, 8, agent.lay.LD + 4, device="cuda"))
    with pytest.raises(ValueError):
        agent.validate_node_windows(torch.zeros(3, 8, agent.lay.LD, device="cuda"), valid=torch.ones(7))
    # a host replay gives what the device replay of the same rows gives
    tr = synth.transitions("Unicycle", 40, seed=2, env=env)
    host, dev = ReplayMemory(64, 0), DeviceReplayMemory(64, 0, agent)
    for i in range(40):                                # chains of 7 transitions: each starts at an observation of its own
        row = [tr[f][i] for f in synth.FIELDS[:8]]
        if i % 7:
            row[synth.FIELDS.index("obs")] = tr["next_obs"][i - 1]
        host.push(*row, t=0.02 * i, next_t=0.02 * (i + 1))
        dev.push(*row, t=0.02 * i, next_t=0.02 * (i + 1))
    idx = torch.arange(40)
    state = random.getstate()
    a, na = agent.validate_node(host, 40, horizon=3, idx=idx)
    assert random.getstate() == state
    b, nb = agent.validate_node(dev, 40, horizon=3, idx=idx)
    assert int(na) == int(nb) and 0 < int(na) < 40
    close(a.cpu().numpy(), b.cpu().numpy(), "host replay vs device replay")      # (float64 -> float32 rows either way)


# ---------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------
def vector_run(every, handover, iters=40, N=64):
    from nlbac_amd.envs import device as denv
    from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory
    from nlbac_amd.train import train_vectorized
    agent, _ = make_agent(64, 64, 0, "euler", "Unicycle", GAMMA_B["Unicycle"])
    env = denv.make("Unicycle", N, seed=0)
    env.max_episode_steps = 25
    args = types.SimpleNamespace(replay_size=4096, seed=0, start_steps=4 * N, batch_size=64, updates_per_step=1,
                                 NODE_model_update_interval=10)
    if every:
        args.node_validate_every, args.node_validate_windows = every, 300
    memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    lines = []
    res = train_vectorized(agent, env, args, iters * N, log=lambda s, *a: lines.append(s), memory=memory, handover=handover)
    torch.cuda.synchronize()
    return agent, memory, res, lines


@pytest.mark.parametrize("handover", [None, True])
def test_vectorised_driver_with_validation_trains_bit_for_bit(handover):
    iters, N, K = 40, 64, 5
    a0, m0, r0, _ = vector_run(0, handover)
    a1, m1, r1, lines = vector_run(K, handover)
    records = r1.pop("node_validation")
    assert "node_validation" not in r0 and r0 == r1
    assert torch.equal(m0.rows, m1.rows) and (m0.position, len(m0), m0._draws) == (m1.position, len(m1), m1._draws)
    for x, y in zip(arenas_of(a0), arenas_of(a1)):
        assert torch.equal(x, y), "validation changed the training run"
    assert torch.equal(a0.sc, a1.sc)
    # update u comes behind vector step u + 2, when the replay holds 64 (u + 2) rows; a window of 3 steps 64 rows apart
    # needs more than 128 of them
    assert r1["updates"] == iters - 1
    due = [u for u in range(0, r1["updates"], K) if N * (u + 2) > 2 * N]
    assert [r["updates"] for r in records] == due and len(due) == 7
    for r in records:
        assert r["rmse"].shape == (3, 3) and r["skill"].shape == (3, 3) and r["rmse_step"].shape == (3,)
        assert 0 <= r["windows_valid"] <= r["windows"] == 300
        assert (r["horizon"], r["stride"], r["solver"], r["steps"]) == (3, N, "euler", N * (r["updates"] + 2))
        assert bool(torch.isfinite(r["rmse"]).all()) if r["windows_valid"] else True
    assert any(r["windows_valid"] > 0 for r in records)
    assert sum(1 for s in lines if s.startswith("node validation:")) == len(records)


def test_host_driver_with_validation_trains_bit_for_bit(tmp_path):
    from nlbac_amd import train
    argv = ["--env", "Unicycle", "--cuda", "--batch_size", "64", "--start_steps", "100", "--max_episodes", "2",
            "--max_steps", "200", "--seed", "0", "--updates_per_step", "1", "--solver", "rk4", "--device_replay"]
    tsv = tmp_path / "validation.tsv"
    runs = []
    for extra in ([], ["--node_validate_every", "5", "--node_validate_windows", "200", "--node_validate_tsv", str(tsv)]):
        seen, records = [], []
        orig = train.train

        def spy(agent, env, dm, args, memory, node_memory, **k):
            seen.append((agent, memory, node_memory))
            return orig(agent, env, dm, args, memory, node_memory, log=QUIET, validation=records, **k)
        train.train = spy
        try:
            hist = train.main(argv + extra)
        finally:
            train.train = orig
        torch.cuda.synchronize()
        agent, memory, node_memory = seen[0]
        runs.append(([{k: v for k, v in h.items() if k != "seconds"} for h in hist], arenas_of(agent), agent.sc.clone(),
                     memory.rows.clone(), node_memory.rows.clone(), records))
    (h0, a0, s0, m0, n0, rec0), (h1, a1, s1, m1, n1, rec1) = runs
    assert h0 == h1 and torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(n0, n1)
    assert all(torch.equal(x, y) for x, y in zip(a0, a1))
    updates = h1[-1]["updates"]
    assert rec0 == [] and [r["updates"] for r in rec1] == list(range(0, updates, 5)) and updates > 100
    for r in rec1:
        assert r["rmse"].shape == (3, 3) and 0 < r["windows_valid"] <= r["windows"] == 200 and r["stride"] == 1
    lines = tsv.read_text().splitlines()
    assert len(lines) == 1 + len(rec1) * 3 * 3
