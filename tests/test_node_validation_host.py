"""Host-side checks of the NODE validation (``node_fit.traj_error_stats`` / ``error_report`` / ``validate_rollout``,
``SAC_CBF_CLF.validate_node``, ``--node_validate_*``): the report against hand-computed numbers, every argument
refusal before a device is touched, the C ABI's declaration, export and refusals of ``nlbac_traj_err_stats``, the
command line, and drivers that never validate with the option off (no GPU needed)."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from nlbac_amd import _lib, node_fit, train
from test_rollout_concat_host import refused

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nlbac_hip.h")


# ---------------------------------------------------------------------------------------------------------------------
# error_report
# ---------------------------------------------------------------------------------------------------------------------
def test_error_report_against_hand_computed_numbers():
    # H = 2, n_s = 2, V = 4
    sse = [[4.0, 16.0], [1.0, 0.0]]
    sae = [[2.0, 8.0], [1.0, 0.0]]
    mx = [[1.5, 3.0], [1.0, 0.0]]
    base = [[8.0, 16.0], [0.0, 4.0]]          # base == 0 at (1, 0)
    tss = [[16.0, 64.0], [4.0, 1.0]]
    stats = torch.tensor([sse, sae, mx, base, tss], dtype=torch.float64)
    r = node_fit.error_report(stats, 4, updates=7, solver="rk4")
    assert r["windows_valid"] == 4 and r["updates"] == 7 and r["solver"] == "rk4"
    assert r["rmse"].tolist() == [[1.0, 2.0], [0.5, 0.0]]
    assert r["mae"].tolist() == [[0.5, 2.0], [0.25, 0.0]]
    assert r["max_abs"].tolist() == mx
    assert r["skill"][0].tolist() == [0.5, 0.0] and math.isnan(float(r["skill"][1, 0])) and float(r["skill"][1, 1]) == 1.0
    assert r["nrmse"].tolist() == [[0.5, 0.5], [0.5, 0.0]]
    np.testing.assert_allclose(r["rmse_step"].numpy(), [math.sqrt(20.0 / 8.0), math.sqrt(1.0 / 8.0)], rtol=1e-15)
    assert r["mse"] == 21.0 / 16.0
    assert r["rmse"].dtype == torch.float64 and r["rmse"].shape == (2, 2) and r["rmse_step"].shape == (2,)
    # the count as a tensor, the statistics as an array
    r2 = node_fit.error_report(stats.numpy(), torch.tensor(4))
    assert r2["mse"] == r["mse"] and torch.equal(r2["rmse"], r["rmse"])
    with pytest.raises(ValueError, match="meta"):
        node_fit.error_report(stats, 4, rmse=1)
    with pytest.raises(ValueError):
        node_fit.error_report(stats[:4], 4)


def test_error_report_without_a_valid_window():
    r = node_fit.error_report(torch.zeros(5, 3, 2, dtype=torch.float64), 0)
    assert r["windows_valid"] == 0
    for k in ("rmse", "mae", "skill", "nrmse", "rmse_step"):
        assert bool(r[k].isnan().all()), k
    assert math.isnan(r["mse"])
    assert r["max_abs"].tolist() == [[0.0, 0.0]] * 3


# ---------------------------------------------------------------------------------------------------------------------
# refusals before a device is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_traj_error_stats_refuses_before_the_device():
    f = node_fit.traj_error_stats
    p, x = torch.zeros(2, 4, 3), torch.zeros(4, 3)
    with pytest.raises(TypeError, match="pred"):
        f(p.double(), p, x)
    with pytest.raises(TypeError, match="target"):
        f(p, p[0], x)
    with pytest.raises(TypeError, match="target"):
        f(p, np.zeros((2, 4, 3), dtype=np.float32), x)
    with pytest.raises(TypeError, match="x0"):
        f(p, p, p)
    with pytest.raises(TypeError, match="x0"):
        f(p, p, x.double())
    with pytest.raises(ValueError, match="same non-empty shape"):
        f(p, torch.zeros(2, 5, 3), x)
    with pytest.raises(ValueError, match="same non-empty shape"):
        f(torch.zeros(0, 4, 3), torch.zeros(0, 4, 3), x)
    with pytest.raises(ValueError, match="x0 must be"):
        f(p, p, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="state components"):
        f(torch.zeros(2, 4, 17), torch.zeros(2, 4, 17), torch.zeros(4, 17))
    with pytest.raises(ValueError, match="one entry per window"):
        f(p, p, x, valid=torch.ones(5))
    with pytest.raises(ValueError, match="CUDA"):          # CPU tensors with everything else in order: the last check
        f(p, p, x, valid=torch.ones(4))


def test_validate_rollout_refuses_before_the_device():
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    f = node_fit.validate_rollout
    s, c = torch.zeros(4, 8, 3), torch.zeros(3, 8, 2)
    with pytest.raises(ValueError, match="states"):
        f(None, s, torch.zeros(4, 8, 2), "rk4", 0.02)
    with pytest.raises(ValueError, match="states"):
        f(None, s[0], c, "rk4", 0.02)
    with pytest.raises(ValueError, match="one entry per window"):
        f(None, s, c, "rk4", 0.02, valid=torch.ones(7))
    with pytest.raises(ValueError, match="state components"):
        f(None, torch.zeros(4, 8, 17), c, "rk4", 0.02)
    with pytest.raises(TypeError, match="NeuralODEModel"):                 # rollout's own refusals, unchanged
        f(torch.nn.Linear(3, 3), s, c, "rk4", 0.02)
    torch.manual_seed(0)
    m = NeuralODEModel(3, 3, 6)           # (host parameters only: attached to no device)
    assert m.affine and m.n_s == 3 and m.n_u == 2
    with pytest.raises(ValueError, match="method is one of"):
        f(m, s, c, "midpoint", 0.02)
    with pytest.raises(ValueError, match="dt must be"):
        f(m, s, c, "rk4", -0.02)
    with pytest.raises(ValueError, match="step_size goes with"):
        f(m, s, c, "dopri5", 0.02, step_size=0.01)
    with pytest.raises(ValueError, match="controls must be"):
        f(m, s, torch.zeros(3, 8, 5), "rk4", 0.02)
    with pytest.raises(ValueError, match="step_control is one of"):
        f(m, s, c, "dopri5", 0.02, step_control="row")
    with pytest.raises(ValueError, match="step_control='tile' goes with"):
        f(m, s, c, "rk4", 0.02, step_control="tile")


class _FakeAgent:
    node_horizon, node_stride, world = 2, 1, 1

    def __getattr__(self, name):
        raise AssertionError("validate_node touched %r before refusing" % name)


class _NoReplay:
    def __len__(self):
        raise AssertionError("validate_node looked at the replay before refusing")


def test_validate_node_refuses_before_the_device():
    from nlbac_amd.sac_cbf_clf.sac_cbf_clf import SAC_CBF_CLF
    f = lambda *a, **k: SAC_CBF_CLF.validate_node(_FakeAgent(), *a, **k)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_windows"):
            f(_NoReplay(), bad)
        with pytest.raises(ValueError, match="horizon"):
            f(_NoReplay(), 8, horizon=bad)
        with pytest.raises(ValueError, match="stride"):
            f(_NoReplay(), 8, stride=bad)
    with pytest.raises(ValueError, match="idx"):
        f(_NoReplay(), 8, idx=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="idx"):
        f(_NoReplay(), 8, idx=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="generator"):
        f(_NoReplay(), 8, generator=np.random.RandomState(0))
    sharded = _FakeAgent()
    sharded.world = 2
    with pytest.raises(RuntimeError, match="node_horizon"):
        SAC_CBF_CLF.validate_node(sharded, _NoReplay(), 8)
    with pytest.raises(RuntimeError, match="node_horizon"):
        SAC_CBF_CLF.validate_node_windows(sharded, torch.zeros(2, 8, 4))
    # a replay shorter than one window: None, and nothing else is touched
    class Short:
        def __len__(self):
            return 4
    assert f(Short(), 8, horizon=3, stride=2) is None
    assert f(Short(), 8, horizon=5) is None


def test_host_replay_windows_at_is_sample_windows_without_a_draw():
    import random
    from nlbac_amd.sac_cbf_clf.replay_memory import ReplayMemory
    mem = ReplayMemory(64, 0)
    obs = 0.0
    for k in range(20):
        nobs = obs + 1.0
        mem.push(np.full(3, obs), np.zeros(2), 0.0, 0.0, np.zeros(2), np.zeros(2), np.full(3, nobs), 1.0, t=k, next_t=k + 1)
        obs = 0.0 if k == 9 else nobs                  # a reset after the tenth push
    random.seed(5)
    state = random.getstate()
    fields, valid = mem.windows_at(np.arange(20), 3)
    assert random.getstate() == state
    assert fields[0].shape == (3, 20, 3) and valid.shape == (20,)
    assert valid.tolist() == [k <= 7 or 10 <= k <= 17 for k in range(20)]
    assert fields[-2][:, 2].tolist() == [2.0, 3.0, 4.0]
    with pytest.raises(ValueError, match="spans more"):
        mem.windows_at(np.arange(4), 21)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_entry_point_is_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    assert re.search(r"\bint\s+nlbac_traj_err_stats\s*\(", text)
    assert "nlbac_traj_err_stats" in _lib.EXPORTS and len(_lib._PROTOS["nlbac_traj_err_stats"]) == 12
    assert lib.nlbac_traj_err_stats is not None
    assert lib.nlbac_abi_version() == 17 == _lib.ABI_VERSION
    assert node_fit.stats_blocks(1, 1) == 1 and node_fit.stats_blocks(1025, 16) == 9
    assert node_fit.stats_blocks(1 << 20, 16) == 128
    assert node_fit.stats_scratch_doubles(7, 1025, 16) == 7 * 9 * 81


def test_entry_point_refuses_bad_arguments(lib):
    host = (C.c_double * 4096)()                 # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    kw = dict(pred=p, target=p, x0=p, valid=None, n=8, H=2, n_s=3, scratch=p, scratch_doubles=4096, stats=p, nvalid=p,
              s=None)
    name = "nlbac_traj_err_stats"
    for key in ("pred", "target", "x0", "scratch", "stats", "nvalid"):
        assert "null" in refused(lib, name, dict(kw, **{key: None}), "a null %s" % key)
    assert "n_s" in refused(lib, name, dict(kw, n_s=17), "n_s = 17")
    assert "n_s" in refused(lib, name, dict(kw, n_s=0), "n_s = 0")
    assert "H must" in refused(lib, name, dict(kw, H=0), "H = 0")
    assert "n must" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "n must" in refused(lib, name, dict(kw, n=1 << 31), "n = 2^31")
    assert "scratch" in refused(lib, name, dict(kw, scratch_doubles=2 * 16 - 1), "a scratch one double short")


# ---------------------------------------------------------------------------------------------------------------------
# command line and drivers
# ---------------------------------------------------------------------------------------------------------------------
def test_the_options_parse():
    a = train.get_args([])
    assert (a.node_validate_every, a.node_validate_windows, a.node_validate_horizon, a.node_validate_tsv) == (0, 4096, None, None)
    assert train.NodeValidation.make(object(), a) is None
    a = train.get_args(["--node_validate_every", "100"])
    v = train.NodeValidation.make(object(), a)
    assert (v.every, v.windows, v.horizon, v.tsv) == (100, 4096, 3, None)          # max(node_horizon, 3)
    assert v.due(0) and v.due(300) and not v.due(150)
    a = train.get_args(["--node_validate_every", "5", "--node_horizon", "6", "--node_validate_windows", "300",
                        "--node_validate_tsv", "v.tsv"])
    v = train.NodeValidation.make(object(), a)
    assert (v.every, v.windows, v.horizon, v.tsv) == (5, 300, 6, "v.tsv")
    a = train.get_args(["--node_validate_every", "5", "--node_horizon", "6", "--node_validate_horizon", "2"])
    assert train.NodeValidation.make(object(), a).horizon == 2
    with pytest.raises(ValueError):
        train.NodeValidation.make(object(), train.get_args(["--node_validate_every", "-1"]))
    with pytest.raises(ValueError):
        train.NodeValidation.make(object(), train.get_args(["--node_validate_every", "1", "--node_validate_windows", "0"]))
    assert train.NodeValidation.make(object(), None) is None                      # (drivers called without args)


def _host_driver(every, calls):
    from nlbac_amd import envs
    from oracle.gen_driver_golden import Recorder, ScriptedAgent
    env = envs.make("Unicycle", 0)
    env.max_episode_steps = 30
    agent = ScriptedAgent("Unicycle", env.action_space)
    agent.validate_node = lambda memory, n, horizon=None: calls.append((memory, n, horizon, agent.updates))
    args = types.SimpleNamespace(env="Unicycle", batch_size=16, updates_per_step=2, start_steps=10, max_episodes=2,
                                 NODE_model_update_interval=10, output=None, max_steps=0)
    if every is not None:
        args.node_validate_every, args.node_validate_windows = every, 77
    mem, node, records = Recorder(), Recorder(), []
    hist = train.train(agent, env, None, args, mem, node, log=lambda *a: None, validation=records)
    return agent, node, hist, records


def test_train_validates_only_with_the_option_on():
    for every in (None, 0):
        calls = []
        _, _, hist, records = _host_driver(every, calls)
        assert calls == [] and records == [] and len(hist) == 2
    calls = []
    agent, node, hist, records = _host_driver(5, calls)
    assert agent.updates == 2 * (60 - 17) and hist[-1]["updates"] == agent.updates
    # before every update whose index is a multiple of 5, on the NODE replay (the stand-in returns None: no record)
    assert [c[3] for c in calls] == list(range(0, agent.updates, 5))
    assert all(c[0] is node and c[1] == 77 and c[2] == 3 for c in calls) and records == []


class _FakeVectorEnv:
    """Four lanes on the host whose episodes never end."""
    n, dt, max_episode_steps = 4, 0.02, 1000

    def __init__(self):
        self.action_space = types.SimpleNamespace(low=np.array([-1.0, -1.0]), high=np.array([1.0, 1.0]))
        self.ep_step = torch.zeros(4, dtype=torch.int32)

    def reset(self):
        return torch.zeros(4, 3, dtype=torch.float64)

    def step(self, action):
        self.ep_step = self.ep_step + 1
        z = torch.zeros(4, dtype=torch.float64)
        return torch.zeros(4, 3, dtype=torch.float64), z, z, torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32), {}

    def reset_done(self, done):
        return torch.zeros(4, 3)


class _FakeReplay:
    def __init__(self):
        self.n = 0

    def push_rows(self, rows):
        self.n += rows.shape[0]

    def __len__(self):
        return self.n


def _vector_driver(every, calls, monkeypatch):
    from nlbac_amd.sac_cbf_clf.tasks import _Task
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    lay = types.SimpleNamespace(sig=None, LD=20, obs=0, obs_dim=3, act=3, act_dim=2, rew=5, con=6, lya=7, lya_dim=2, nlya=9,
                                nobs=11, mask=14, t=15, nt=16)
    agent = types.SimpleNamespace(device=torch.device("cpu"), lay=lay, node_stride=1, solver="euler", updates=0,
                                  task=type("T", (), {"fit_due": _Task.fit_due})())
    agent.update_parameters = lambda *a: setattr(agent, "updates", agent.updates + 1)
    agent.validate_node = lambda memory, n, horizon=None: calls.append((memory, n, horizon, agent.updates))
    args = types.SimpleNamespace(replay_size=64, seed=0, start_steps=1 << 30, batch_size=8, updates_per_step=1,
                                 NODE_model_update_interval=10)
    if every is not None:
        args.node_validate_every = every
    memory = _FakeReplay()
    res = train.train_vectorized(agent, _FakeVectorEnv(), args, 4 * 20, log=lambda *a: None, memory=memory)
    return agent, memory, res


def test_train_vectorized_validates_only_with_the_option_on(monkeypatch):
    for every in (None, 0):
        calls = []
        agent, _, res = _vector_driver(every, calls, monkeypatch)
        assert calls == [] and agent.updates == 18 and "node_validation" not in res
        assert res == dict(steps=80, updates=18, episodes=0, mean_return=0.0)
    calls = []
    agent, memory, res = _vector_driver(4, calls, monkeypatch)
    assert [c[3] for c in calls] == [0, 4, 8, 12, 16] and all(c[0] is memory and c[1] == 4096 and c[2] == 3 for c in calls)
    assert res.pop("node_validation") == [] and agent.node_stride == 4
    assert res == dict(steps=80, updates=18, episodes=0, mean_return=0.0)


def test_validation_tsv(tmp_path):
    stats = torch.arange(1.0, 31.0, dtype=torch.float64).reshape(5, 2, 3)
    recs = [node_fit.error_report(stats, 9, updates=10 * i, steps=40 * i, horizon=2, stride=4, windows=12, solver="rk4")
            for i in range(2)]
    path = tmp_path / "v.tsv"
    train.write_validation_tsv(str(path), recs)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(train.NodeValidation.TSV_COLUMNS) and len(lines) == 1 + 2 * 2 * 3
    row = dict(zip(lines[0].split("\t"), lines[1 + 6 + 4].split("\t")))            # record 1, k = 2, c = 1
    assert (row["updates"], row["steps"], row["k"], row["c"], row["solver"], row["windows_valid"]) == ("10", "40", "2", "1", "rk4", "9")
    assert float(row["rmse"]) == float(recs[1]["rmse"][1, 1]) and float(row["skill"]) == float(recs[1]["skill"][1, 1])
