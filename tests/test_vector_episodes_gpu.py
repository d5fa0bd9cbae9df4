"""GPU: the vectorised driver's per-episode ledger (``nlbac_amd.vector_episodes``, ``train.train_vectorized(
episodes=...)``, ``train.evaluate_vectorized``).  The records against numpy over the reference driver's own traces, bit
for bit and in (vector step, lane) order; the ranks across workgroups, a ragged last workgroup and a ring that wraps; a
run with the option against the same run without it; the launches of a vector step; the evaluation pass."""
import os
import types

import numpy as np
import pytest
import torch

from nlbac_amd import _lib, vector_handover
from nlbac_amd.envs import device as denv
from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory
from nlbac_amd.train import evaluate_vectorized, train_vectorized
from nlbac_amd.vector_episodes import HISTORY_KEYS, EpisodeLedger

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("reward", "safety_cost", "violations", "length", "goal_met", "timeout", "backup_steps", "lane", "lane_episode",
          "vstep", "updates")


def same_records(arrays, want, what=""):
    """``arrays`` (``EpisodeLedger.records``) against a list of expected records (dicts of ``FIELDS``), exactly."""
    assert len(arrays["episode"]) == len(want), "%s%d records, expected %d" % (what, len(arrays["episode"]), len(want))
    for f in FIELDS:
        got, exp = arrays[f], np.array([w[f] for w in want], dtype=arrays[f].dtype)
        bad = np.flatnonzero(got != exp)                                     # (float64 ==: no tolerance anywhere)
        assert len(bad) == 0, "%s%s: first differing record %d: got %r, expected %r" % (what, f, bad[0], got[bad[0]], exp[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the reference's own loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["Unicycle", "Pvtol", "SimulatedCars", "SimulatedCarsHandover"])
def test_records_are_numpy_over_the_reference_traces(fixture):
    g = np.load(os.path.join(GOLD, "driver_%s.npz" % fixture))
    done = g["done"].astype(bool)
    ends = np.flatnonzero(done)
    assert ends[-1] == len(done) - 1
    starts = np.concatenate([[0], ends[:-1] + 1])
    E, N, max_steps = len(ends), 70, int(g["meta_max_steps"])                # (two waves, the second ragged)
    first = g["reached"] if fixture.startswith("SimulatedCars") else g["goal_met"]
    T = len(done) - 37                                                       # (every lane ends inside an episode)
    order = [np.concatenate([np.arange(starts[e % E], ends[e % E] + 1) for e in range(r, r + E)])[:T] for r in range(E)]
    assert not any(done[o][-1] for o in order)
    # expected, per rotation: numpy over the done-delimited segments (cumsum adds in step order)
    per_rotation = []
    for o in order:
        recs, s = [], 0
        for e in np.flatnonzero(done[o]):
            seg = o[s:e + 1]
            recs.append(dict(reward=np.cumsum(g["reward"][seg])[-1], safety_cost=np.cumsum(g["safety_cost"][seg])[-1],
                             violations=int(np.cumsum(g["n_violation"][seg])[-1]), length=len(seg),
                             goal_met=int(first[seg[-1]] != 0), timeout=int(len(seg) >= max_steps),
                             backup_steps=int(g["backup"][seg].sum()), lane_episode=len(recs), vstep=int(e),
                             updates=3 * int(e) + 1))
            s = e + 1
        per_rotation.append((recs, o[s:]))
    want = sorted((dict(r, lane=j) for j in range(N) for r in per_rotation[j % E][0]), key=lambda r: (r["vstep"], r["lane"]))
    tails = [per_rotation[j % E][1] for j in range(N)]
    # the replay: lane j walks rotation j mod E
    lane_order = np.stack([order[j % E] for j in range(N)], axis=1)          # (T, N) trace step of lane j at step t
    dev = torch.device("cuda")
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a[lane_order]), dtype=dt, device=dev)
    k = np.concatenate([np.arange(1, e - s + 2) for s, e in zip(starts, ends)])        # ep_step, rebuilt from done
    info = up(np.stack([first, g["n_violation"], g["safety_cost"]], axis=1), torch.float64)      # (T, N, 3)
    reward, dn, kk, flags = up(g["reward"], torch.float64), up(done, torch.int32), up(k, torch.int32), up(g["backup"] != 0, torch.bool)
    led = EpisodeLedger(N, dev)
    for t in range(T):
        led.push(reward[t], dn[t], info[t], kk[t], max_steps, flags=flags[t], vstep=t, updates=3 * t + 1)
    arrays, history = led.records()
    assert arrays["total"] == len(want) == sum(len(per_rotation[j % E][0]) for j in range(N)) > 0
    same_records(arrays, want)
    assert [tuple(h) for h in history] == [HISTORY_KEYS] * len(want) and history[-1]["total_steps"] == (want[-1]["vstep"] + 1) * N
    assert led.lane_episodes.cpu().tolist() == [len(per_rotation[j % E][0]) for j in range(N)]
    # the trailing segment without ``done`` yields no record: its steps are the open ones
    tot = led.totals()
    assert tot["episodes"] == len(want) and tot["steps"] + tot["open_steps"] == T * N
    assert tot["open_steps"] == sum(len(s) for s in tails) > 0
    assert tot["open_backup_steps"] == sum(int(g["backup"][s].sum()) for s in tails)
    assert tot["backup_steps"] == sum(r["backup_steps"] for r in want)
    assert tot["backup_steps"] + tot["open_backup_steps"] == int(g["backup"][lane_order].sum())
    assert tot["violations"] == sum(r["violations"] for r in want)
    assert tot["open_violations"] == sum(int(g["n_violation"][s].sum()) for s in tails)
    assert tot["open_reward"] == float(np.array([np.cumsum(g["reward"][s])[-1] for s in tails]).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 2. several workgroups, a ragged end, a ring that wraps
# ---------------------------------------------------------------------------------------------------------------------
def host_ledger(reward, info, done, flags, ep_step, max_steps, updates):
    """A host loop over the same numbers: the records in (step, lane) order and the per-lane sums over finished episodes."""
    T, N = reward.shape
    ret, cost, viol = np.zeros(N), np.zeros(N), np.zeros(N)
    length, backup, episodes = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    life = dict(reward=np.zeros(N), safety_cost=np.zeros(N), violations=np.zeros(N), steps=np.zeros(N, dtype=np.int64),
                backup_steps=np.zeros(N, dtype=np.int64))
    recs = []
    for t in range(T):
        ret, viol, cost = ret + reward[t], viol + info[t, :, 1], cost + info[t, :, 2]
        length, backup = length + 1, backup + flags[t]
        for i in np.flatnonzero(done[t]):
            recs.append(dict(reward=ret[i], safety_cost=cost[i], violations=int(viol[i]), length=int(length[i]),
                             goal_met=int(info[t, i, 0] != 0), timeout=int(ep_step[t, i] >= max_steps),
                             backup_steps=int(backup[i]), lane=int(i), lane_episode=int(episodes[i]), vstep=t,
                             updates=int(updates[t])))
            life["reward"][i] = life["reward"][i] + ret[i]
            life["safety_cost"][i] = life["safety_cost"][i] + cost[i]
            life["violations"][i] = life["violations"][i] + viol[i]
            life["steps"][i] += length[i]
            life["backup_steps"][i] += backup[i]
            ret[i] = cost[i] = viol[i] = 0.0
            length[i] = backup[i] = 0
            episodes[i] += 1
    return recs, life, dict(open_steps=int(length.sum()), open_backup_steps=int(backup.sum()), open_reward=float(ret.sum()),
                            open_safety_cost=float(cost.sum()), open_violations=int(viol.sum()))


def random_steps(rng, T, N, p, none_at=None, all_at=None):
    done = rng.random((T, N)) < p
    if none_at is not None:
        done[none_at] = False
    if all_at is not None:
        done[all_at] = True
    reward = rng.normal(size=(T, N)) * 10.0 ** rng.integers(-3, 4, size=(T, N))        # (sums that do round)
    info = np.zeros((T, N, 3))
    info[:, :, 0] = rng.random((T, N)) < 0.5
    info[:, :, 1] = rng.integers(0, 4, size=(T, N))
    info[:, :, 2] = rng.random((T, N))
    flags = rng.random((T, N)) < 0.4
    ep_step = np.zeros((T, N), dtype=np.int32)
    run = np.zeros(N, dtype=np.int32)
    for t in range(T):
        run += 1
        ep_step[t] = run
        run[done[t]] = 0
    return reward, info, done, flags, ep_step


def replay(led, reward, info, done, flags, ep_step, max_steps, updates, first_key_column=0):
    dev = led.device
    T, N = reward.shape
    block = np.zeros((T, N, first_key_column + 3))
    block[:, :, :first_key_column] = -7.0                                    # (columns the ledger must not read)
    block[:, :, first_key_column:] = info
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    r, b, d, f, k = up(reward, torch.float64), up(block, torch.float64), up(done, torch.int32), up(flags, torch.uint8), up(ep_step, torch.int32)
    for t in range(T):
        led.push(r[t], d[t], b[t], k[t], max_steps, first_key_column=first_key_column, flags=f[t], vstep=t, updates=int(updates[t]))


def test_ranks_across_workgroups_a_ragged_end_and_a_ring_that_wraps():
    N, T, cap, max_steps = 600, 40, 1024, 4                                  # workgroups of 256, 256 and 88 lanes
    rng = np.random.default_rng(11)
    steps = random_steps(rng, T, N, 0.3, none_at=7, all_at=23)               # workgroup counts 0 and 256 / 88
    updates = np.arange(T) * 2
    want, life, open_ = host_ledger(*steps, max_steps, updates)
    assert 6500 < len(want) < 8000 and len(want) > 6 * cap
    assert {r["timeout"] for r in want} == {0, 1}
    led = EpisodeLedger(N, "cuda", capacity=cap)
    replay(led, *steps, max_steps, updates, first_key_column=2)
    arrays, history = led.records(since=len(want) - cap)
    assert arrays["total"] == len(want)
    assert arrays["episode"].tolist() == list(range(len(want) - cap, len(want)))
    same_records(arrays, want[-cap:])
    assert led.head.cpu().tolist()[led.half] == [len(want) % cap, len(want)]
    for since in (0, len(want) - cap - 1):
        with pytest.raises(ValueError, match="capacity"):
            led.records(since=since)
    same_records(led.records(since=len(want) - 5)[0], want[-5:])
    tot = led.totals()
    assert tot["episodes"] == len(want) and tot["steps"] == int(life["steps"].sum())
    assert tot["backup_steps"] == int(life["backup_steps"].sum()) and tot["violations"] == int(life["violations"].sum())
    assert tot["reward"] == float(life["reward"].sum()) and tot["safety_cost"] == float(life["safety_cost"].sum())
    assert {k: tot[k] for k in open_} == open_ and tot["steps"] + tot["open_steps"] == T * N
    assert led.lane_episodes.cpu().tolist() == np.sum(steps[2], axis=0).tolist()


@pytest.mark.parametrize("N", [1, 64, 65536])
def test_the_narrowest_and_the_widest_ledger(N):
    """1 lane, one full wave and 256 full workgroups (the most ``counts`` a workgroup sums), without flags."""
    T, max_steps = 4, 3
    rng = np.random.default_rng(N)
    reward, info, done, flags, ep_step = random_steps(rng, T, N, 0.3, all_at=2)
    updates = np.arange(T) + 5
    want, life, open_ = host_ledger(reward, info, done, np.zeros_like(flags), ep_step, max_steps, updates)
    led = EpisodeLedger(N, "cuda", capacity=max(N, len(want)))
    dev = led.device
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    r, b, d, k = up(reward, torch.float64), up(info, torch.float64), up(done, torch.int32), up(ep_step, torch.int32)
    for t in range(T):
        led.push(r[t], d[t], b[t], k[t], max_steps, vstep=t, updates=int(updates[t]))
    same_records(led.records()[0], want)
    tot = led.totals()
    assert tot["backup_steps"] == tot["open_backup_steps"] == 0 and tot["episodes"] == len(want)
    assert tot["reward"] == float(life["reward"].sum()) and tot["open_steps"] == open_["open_steps"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the option changes nothing / 4. no extra launches without it
# ---------------------------------------------------------------------------------------------------------------------
N_LANES, ITERS, MAX_STEPS, BATCH = 64, 240, 20, 64
_RUNS = {}


def run(handover, episodes):
    """One vectorised training run (cached: the cases below share four of them); the library calls of every vector
    step are recorded on the way."""
    key = (handover, episodes)
    if key in _RUNS:
        return _RUNS[key]
    from test_agent_parity_gpu import make_agent
    torch.manual_seed(0)
    agent, _ = make_agent(BATCH, 64, 0, "euler", "Unicycle", 50.0)
    env = denv.make("Unicycle", N_LANES, seed=0)
    env.max_episode_steps = MAX_STEPS
    args = types.SimpleNamespace(replay_size=4096, seed=0, start_steps=4 * N_LANES, batch_size=BATCH, updates_per_step=1,
                                 NODE_model_update_interval=10)
    memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    kw = {}
    if handover:       # a hand-over that does fire within 20-step episodes: stuck after one check at step 5, back after 3
        kw["handover"] = vector_handover.params_for("Unicycle", env, first_backup_episode=1, min_check_step=5, lookback=5,
                                                    checks=1, stuck2=1e9, away2=1e9, max_backup=3)
    names, marks, real = [], [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        res = train_vectorized(agent, env, args, ITERS * N_LANES, log=lambda *a: None, memory=memory,
                               check=lambda it, *a: marks.append(len(names)), episodes=episodes, **kw)
    finally:
        _lib.call = real
    torch.cuda.synchronize()
    per_step = [names[a:b] for a, b in zip(marks[:-1], marks[1:])]           # (check k-1 .. check k: one vector step)
    _RUNS[key] = (agent, memory, res, per_step)
    return _RUNS[key]


@pytest.mark.parametrize("handover", [False, True], ids=["plain", "handover"])
def test_the_option_changes_nothing(handover):
    a0, m0, r0, _ = run(handover, None)
    a1, m1, r1, _ = run(handover, True)
    new = {"history", "violations", "safety_cost", "ledger"}
    assert set(r1) - set(r0) == new and not new & set(r0)
    assert {k: r1[k] for k in r0} == r0, "a key the driver had before changed its value"
    assert r0["steps"] == ITERS * N_LANES and r0["updates"] > ITERS // 2 and r0["episodes"] >= ITERS // MAX_STEPS * N_LANES
    for x, y in zip(a0.arenas, a1.arenas):
        assert torch.equal(x.theta, y.theta), "the run with the ledger differs from the run without"
    assert torch.equal(m0.rows, m1.rows) and (m0.position, len(m0), m0._draws) == (m1.position, len(m1), m1._draws)
    hist, led = r1["history"], r1["ledger"]
    assert len(hist) == r1["episodes"] and isinstance(led, EpisodeLedger)
    assert all(1 <= h["length"] <= MAX_STEPS for h in hist)
    assert all(h["timeout"] == int(h["length"] == MAX_STEPS and h["goal_met"] == 0) for h in hist)
    assert any(h["timeout"] for h in hist)
    total = sum(h["reward"] for h in hist)
    scale = sum(abs(h["reward"]) for h in hist)
    print("sum of history rewards %.17g, mean_return * episodes %.17g, bound %.3g" % (total, r1["mean_return"] * r1["episodes"], 1e-12 * scale))
    assert abs(total - r1["mean_return"] * r1["episodes"]) <= 1e-12 * scale
    tot = led.totals()
    assert r1["violations"] == tot["violations"] == sum(h["violations"] for h in hist)
    assert r1["safety_cost"] == tot["safety_cost"]
    assert abs(sum(h["safety_cost"] for h in hist) - tot["safety_cost"]) <= 1e-12 * max(tot["safety_cost"], 1.0)
    assert sum(h["length"] for h in hist) + tot["open_steps"] == r1["steps"]
    assert [h["episode"] for h in hist] == list(range(len(hist)))
    order = [(h["total_steps"], h["lane"]) for h in hist]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert all(h["total_steps"] % N_LANES == 0 and 0 <= h["updates"] <= r1["updates"] for h in hist)
    assert [h["updates"] for h in hist] == sorted(h["updates"] for h in hist)
    if handover:
        assert r1["backup_steps"] > 0
        assert sum(h["backup_steps"] for h in hist) + tot["open_backup_steps"] == r1["backup_steps"]
        assert tot["backup_steps"] == sum(h["backup_steps"] for h in hist)
    else:
        assert tot["backup_steps"] == tot["open_backup_steps"] == 0 and not any(h["backup_steps"] for h in hist)


@pytest.mark.parametrize("handover", [False, True], ids=["plain", "handover"])
def test_no_extra_launches_without_the_option(handover):
    off, on = run(handover, None)[3], run(handover, True)[3]
    assert len(off) == len(on) == ITERS - 1
    for step in off:
        assert not [n for n in step if n.startswith("nlbac_episode_")]
    for step in on:
        assert step.count("nlbac_episode_step") == 1 and step.count("nlbac_episode_append") == 1
        assert step.index("nlbac_unicycle_env_step") < step.index("nlbac_episode_step") < step.index("nlbac_episode_append")
        if handover:
            assert step.index("nlbac_episode_append") < step.index("nlbac_vector_step_rows")
    strip = lambda step: [n for n in step if not n.startswith("nlbac_episode_")]
    assert [strip(s) for s in on] == off, "with the option off the driver issues other launches than the ledger's two"


def test_a_ledger_handed_in_keeps_counting_and_another_width_is_refused():
    from test_agent_parity_gpu import make_agent
    agent, _ = make_agent(BATCH, 64, 0, "euler", "Unicycle", 50.0)
    args = types.SimpleNamespace(replay_size=4096, seed=0, start_steps=10 ** 9, batch_size=10 ** 9, updates_per_step=1,
                                 NODE_model_update_interval=10)
    for cap in (64, 16):
        led, runs = EpisodeLedger(16, "cuda", capacity=cap), []
        for _ in range(2):
            env = denv.make("Unicycle", 16, seed=0)
            env.max_episode_steps = 5
            runs.append(train_vectorized(agent, env, args, 16 * 10, log=lambda *a: None, episodes=led))
        res = runs[1]
        assert res["ledger"] is led and res["episodes"] == 32 and led.totals()["episodes"] == 64
        if cap == 16:                                                              # (what the ring of 16 still holds)
            assert len(res["history"]) == 16 and res["history"][0]["episode"] == 48
            continue
        # the second run reports what it added, not the ledger's lifetime: the same seeds, and the first run left no
        # episode open (10 steps, episodes of 5), so the same figures; only the ledger's own counters go on
        assert [h["episode"] for h in res["history"]] == list(range(32, 64))
        assert [h["total_steps"] for h in res["history"]] == [h["total_steps"] for h in runs[0]["history"]]
        strip = lambda hist: [{k: v for k, v in h.items() if k not in ("episode", "lane_episode")} for h in hist]
        assert [h["lane_episode"] for h in res["history"]] == [h["lane_episode"] + 2 for h in runs[0]["history"]]
        assert strip(res["history"]) == strip(runs[0]["history"])
        assert res["violations"] == runs[0]["violations"] == sum(h["violations"] for h in res["history"])
        assert abs(res["safety_cost"] - runs[0]["safety_cost"]) <= 1e-12 * max(1.0, runs[0]["safety_cost"])
        tot = led.totals()
        assert tot["violations"] == 2 * res["violations"] and len(led.records()[1]) == 64
    with pytest.raises(ValueError, match="16 lanes, the environment 8"):
        train_vectorized(agent, denv.make("Unicycle", 8, seed=0), args, 8, log=lambda *a: None, episodes=led)


# ---------------------------------------------------------------------------------------------------------------------
# 5. evaluation
# ---------------------------------------------------------------------------------------------------------------------
class ShortEpisodes:
    """A scripted device environment in the simulators' shape whose episodes end — goal met — after ``L`` steps, far
    short of ``max_episode_steps``: reward = lane + step count / 1024 (exact in float64), one violation per step in the
    odd lanes, safety cost 0.5 there."""

    def __init__(self, n, L, max_episode_steps, device="cuda"):
        self.n, self.L, self.max_episode_steps, self.device = n, L, max_episode_steps, torch.device(device)
        z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=self.device)
        self.obs, self.reward, self.info = z(n, 7), z(n), z(n, 3)
        self.ep_step, self.done = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
        self.lane = torch.arange(n, dtype=torch.float64, device=self.device)
        self.info[:, 1] = (torch.arange(n, device=self.device) % 2).double()
        self.info[:, 2] = 0.5 * self.info[:, 1]
        self.t = 0

    def reset(self, mask=None):
        if mask is None:
            self.ep_step.zero_()
            self.t = 0
        else:
            self.ep_step[mask] = 0
        return self.obs

    def step(self, action):
        self.t += 1
        self.ep_step += 1
        self.reward.copy_(self.lane + self.t / 1024.0)
        self.done.copy_((self.ep_step >= self.L).to(torch.int32))
        self.info[:, 0] = self.done.double()
        info = {"goal_met": self.info[:, 0], "num_safety_violation": self.info[:, 1], "safety_cost": self.info[:, 2]}
        return (self.obs, self.reward, self.reward, self.obs, self.obs, self.done, info)


@pytest.mark.parametrize("capacity", [None, 1024, 5000])
def test_evaluation_with_episodes_far_shorter_than_the_time_limit(capacity):
    """1024 lanes whose episodes last 2 steps under a time limit of 400: until the time limit has passed once the lanes
    write 1024 * 400 / 2 = 204 800 records, more than the default ring (65 536) or any ring handed in here holds.  The
    records returned must still be every lane's FIRST two, so the ring is read before it can wrap over them."""
    N, L, max_steps, per_lane = 1024, 2, 400, 2
    env = ShortEpisodes(N, L, max_steps)
    agent = types.SimpleNamespace(device=env.device, lay=types.SimpleNamespace(act_dim=2), policy=types.SimpleNamespace(
        sample=lambda obs, eps=None: (None, None, torch.zeros(N, 2, device=env.device))))
    led = None if capacity is None else EpisodeLedger(N, "cuda", capacity=capacity)
    res = evaluate_vectorized(agent, env, per_lane, ledger=led)
    assert N * max_steps // L > 65536 and res["episodes"] == N * per_lane
    want = [dict(reward=float(i) * L + sum(range(e * L + 1, e * L + L + 1)) / 1024.0, safety_cost=0.5 * L * (i % 2),
                 violations=L * (i % 2), length=L, goal_met=1, timeout=0, backup_steps=0, lane=i, lane_episode=e,
                 vstep=e * L + L - 1, updates=0) for e in range(per_lane) for i in range(N)]
    same_records(res["arrays"], want)
    read_every = (65536 if capacity is None else capacity) // N
    assert res["steps"] == N * max(read_every, -(-per_lane * L // read_every) * read_every)     # (stops at the first read that has them)
    assert res["steps"] < N * max_steps and res["goal_rate"] == 1.0 and res["mean_length"] == L
    assert res["violations_per_episode"] == L * 0.5


def test_evaluation_records_two_episodes_per_lane_and_moves_nothing():
    from test_agent_parity_gpu import make_agent
    agent, _ = make_agent(BATCH, 64, 0, "euler", "Unicycle", 50.0)
    env = denv.make("Unicycle", N_LANES, seed=0)
    env.max_episode_steps = MAX_STEPS
    torch.cuda.synchronize()
    cuda_rng, cpu_rng = torch.cuda.get_rng_state(), torch.get_rng_state()
    arenas = [a.theta.clone() for a in agent.arenas]
    names, real = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        first = evaluate_vectorized(agent, env, episodes_per_lane=2)
    finally:
        _lib.call = real
    second = evaluate_vectorized(agent, env, episodes_per_lane=2)
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), cuda_rng) and torch.equal(torch.get_rng_state(), cpu_rng)
    for a, before in zip(agent.arenas, arenas):
        assert torch.equal(a.theta, before)
    assert not [n for n in names if "adam" in n or "sample_rows" in n or "bwd" in n], "evaluation ran an update"
    assert names.count("nlbac_episode_step") == names.count("nlbac_unicycle_env_step") <= 2 * MAX_STEPS
    hist = first["history"]
    assert first["episodes"] == len(hist) == 2 * N_LANES
    assert sorted((h["lane"], h["lane_episode"]) for h in hist) == [(i, e) for i in range(N_LANES) for e in (0, 1)]
    assert hist == second["history"] and all(np.array_equal(first["arrays"][k], second["arrays"][k]) for k in first["arrays"])
    assert {k: first[k] for k in first if k not in ("history", "arrays")} == {k: second[k] for k in second if k not in ("history", "arrays")}
    ret, length = np.array([h["reward"] for h in hist]), np.array([h["length"] for h in hist], dtype=np.float64)
    assert first["mean_return"] == float(ret.mean()) and first["std_return"] == float(ret.std())
    assert first["mean_length"] == float(length.mean()) and first["std_length"] == float(length.std())
    assert first["violations_per_episode"] == sum(h["violations"] for h in hist) / len(hist)
    assert first["goal_rate"] == sum(h["goal_met"] for h in hist) / len(hist)
    assert all(1 <= h["length"] <= MAX_STEPS and h["updates"] == 0 and h["backup_steps"] == 0 for h in hist)
