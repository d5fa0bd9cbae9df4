"""GPU: start positions drawn per reset for Unicycle, Pvtol and their barrier copies (``envs.device.make(name, n, seed,
device_resets=True, init_spread=(sx, sy))``: ``nlbac_unicycle_env_reset`` / ``nlbac_pvtol_env_reset``) against the numpy
restatement of the draw (tests/test_start_spread_host.py) and the host simulators' ``reset(offset=)``.  Floats agree
within rtol 1e-9 / atol 1e-11, what tests/test_device_envs_gpu.py allows the same tasks' step kernels; the draws within
1e-12, the bar of the Quadrotor-like draw (tests/test_quadrotor_env_gpu.py: the same arithmetic); counters, flags,
``done``, the violation counts and ``goal`` agree exactly.  300 lanes: two workgroups of the 256-thread launch, the
second ragged."""
import numpy as np
import pytest
import torch

from nlbac_amd import _lib, envs
from nlbac_amd.envs import device as D
from nlbac_amd.train import evaluate_vectorized
from test_agent_parity_gpu import make_agent
from test_start_spread_host import START, TASKS, base, start_reset_offsets

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-9, atol=1e-11)          # the simulators' tolerance in tests/test_device_envs_gpu.py
N, SEED, SPREAD = 300, 5, (0.3, 0.2)
NEW = ("nlbac_unicycle_env_reset", "nlbac_pvtol_env_reset")


def flags(mask):
    return torch.as_tensor(np.asarray(mask).astype(np.int32), device="cuda")


def actions(rs, env, *lead):
    lo, hi = np.asarray(env.action_space.low, dtype=np.float64), np.asarray(env.action_space.high, dtype=np.float64)
    return rs.uniform(lo, hi, size=lead + (env.n, env.act_dim))


def float64_tensors(env):
    names = ["state", "obs", "reset_noise", "reward", "constraint", "signal", "lya_pre", "lya_next", "info"]
    return {k: getattr(env, k) for k in names + (["last_dist"] if hasattr(env, "last_dist") else [])}


def host_at(name, offsets):
    """one host simulator per row of ``offsets``, reset there -> (simulators, their observations)"""
    hosts = [envs.make(name, 0) for _ in range(len(offsets))]
    return hosts, np.array([h.reset(offset=o) for h, o in zip(hosts, offsets)])


def check_reset_lanes(name, env, mask, count):
    """the lanes ``mask`` of ``env`` were just reset, each for the ``count``-th time (0: the constructor's)"""
    lanes = np.flatnonzero(mask)
    want = start_reset_offsets(SEED, lanes, count[lanes], *SPREAD)
    state = env.state.cpu().numpy()
    noise = env.reset_noise.cpu().numpy()
    moved = state[lanes, :2] - START[base(name)]
    print("%s: %d lanes reset; largest |offset - numpy restatement| %.3e (state - start: %.3e)"
          % (name, len(lanes), np.abs(noise[lanes] - want).max(), np.abs(moved - want).max()))
    np.testing.assert_allclose(moved, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(noise[lanes], want, rtol=0, atol=1e-12)
    assert (np.abs(noise[lanes]) <= np.array(SPREAD)).all()
    hosts, obs = host_at(name, noise[lanes])
    np.testing.assert_allclose(env.obs.cpu().numpy()[lanes], obs, **TOL)
    np.testing.assert_allclose(state[lanes], np.array([h.state for h in hosts]), **TOL)
    assert np.array_equal(state[lanes], np.array([h.state for h in hosts]))      # (start + offset: one rounded sum)
    if base(name) == "Unicycle":
        np.testing.assert_allclose(env.last_dist.cpu().numpy()[lanes], [h.last_goal_dist for h in hosts], **TOL)
        assert np.array_equal(state[lanes, 2], np.zeros(len(lanes)))
    else:
        assert np.array_equal(state[lanes, 6], state[lanes, 0])                   # the operator starts at the vehicle's x
        assert np.array_equal(state[lanes, 2:6], np.tile([0.0, 0.0, 0.0, 1.0], (len(lanes), 1)))
    assert int(env.ep_step[torch.as_tensor(mask, device="cuda")].abs().max()) == 0
    assert all(h.episode_step == 0 for h in hosts)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reset launch: drawn lanes against numpy and the host simulators, other lanes untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TASKS)
def test_reset_lanes_and_lanes_that_go_on(name):
    env = D.make(name, N, SEED, device_resets=True, init_spread=SPREAD)
    assert env.init_spread == SPREAD and env.reset_noise.shape == (N, 2) and env.obs32.dtype == torch.float32
    count = np.zeros(N, dtype=np.int64)
    every = np.ones(N, dtype=bool)
    check_reset_lanes(name, env, every, count)                       # the constructor's reset
    count += 1
    assert np.array_equal(env.reset_count.cpu().numpy(), count)
    assert torch.equal(env.obs32, env.obs.to(torch.float32))
    first = env.reset_noise.cpu().numpy().copy()
    assert len(np.unique(first[:, 0])) == N and len(np.unique(first[:, 1])) == N         # lane to lane
    rs, rm = np.random.RandomState(3), np.random.RandomState(4)
    for k in range(3):
        for _ in range(2):                                           # (lanes that go on hold the step kernel's values)
            env.step(actions(rs, env))
        mask = rm.rand(N) < 0.4
        mask[[0, 255, 256, N - 1]] = [k == 0, k == 1, k != 1, k == 2]    # both sides of the workgroup edge, both ends
        m = torch.as_tensor(mask, device="cuda")
        before = {key: v.clone() for key, v in float64_tensors(env).items()}
        steps, counts = env.ep_step.clone(), env.reset_count.clone()
        out = env.reset_done(flags(mask))
        torch.cuda.synchronize()
        assert out is env.obs32
        for key, v in float64_tensors(env).items():
            assert torch.equal(v[~m], before[key][~m]), "%s of a lane that was not reset changed" % key
        assert torch.equal(env.ep_step[~m], steps[~m]) and torch.equal(env.reset_count[~m], counts[~m])
        assert bool((env.ep_step[~m] == 2 * (k + 1)).any())          # (some lane has never been reset since the start)
        assert torch.equal(env.obs32, env.obs.to(torch.float32))     # every lane: reset ones and the others' untouched obs
        check_reset_lanes(name, env, mask, count)
        count += mask
        assert np.array_equal(env.reset_count.cpu().numpy(), count)
    # reset to reset the draws differ; a full reset() draws for every lane
    env.reset()
    check_reset_lanes(name, env, every, count)
    assert not (env.reset_noise.cpu().numpy() == first).any()
    # given offsets are honoured (and recorded), also where the environment has no spread of its own
    given = np.stack([np.linspace(-0.25, 0.25, N), np.linspace(0.1, -0.1, N)], axis=1)
    for e in (env, D.make(name, N, SEED, device_resets=True)):
        e.reset(noise=given)
        assert np.array_equal(e.reset_noise.cpu().numpy(), given)
        hosts, obs = host_at(name, given)
        assert np.array_equal(e.state.cpu().numpy(), np.array([h.state for h in hosts]))
        np.testing.assert_allclose(e.obs.cpu().numpy(), obs, **TOL)
        assert torch.equal(e.obs32, e.obs.to(torch.float32))
    with pytest.raises(ValueError, match="device_resets"):
        D.make(name, N, SEED).reset(noise=given)


@pytest.mark.parametrize("name", TASKS)
def test_the_draw_depends_on_seed_lane_and_count_alone(name):
    big = D.make(name, N, SEED, device_resets=True, init_spread=SPREAD)
    small = D.make(name, 64, SEED, device_resets=True, init_spread=SPREAD)
    other = D.make(name, N, SEED + 1, device_resets=True, init_spread=SPREAD)
    for k in range(2):
        for key in ("reset_noise", "state", "obs"):
            assert torch.equal(getattr(small, key), getattr(big, key)[:64]), (key, k)
        assert not bool((other.reset_noise == big.reset_noise).any())
        for e in (big, small, other):
            e.reset()
    # not on when the reset happened either: lanes reset at different times hold their own count's draw
    late = D.make(name, N, SEED, device_resets=True, init_spread=SPREAD)
    mask = np.arange(N) % 2 == 0
    late.reset_done(flags(mask))
    late.reset_done(flags(~mask))
    want = start_reset_offsets(SEED, np.arange(N), 1, *SPREAD)
    np.testing.assert_allclose(late.reset_noise.cpu().numpy(), want, rtol=0, atol=1e-12)
    # the two tasks share the tag: the same seed, lane and count give the same unit draw
    twin = D.make("Pvtol" if base(name) == "Unicycle" else "Unicycle", N, SEED, device_resets=True, init_spread=SPREAD)
    assert torch.equal(twin.reset_noise, D.make(name, N, SEED, device_resets=True, init_spread=SPREAD).reset_noise)


# ---------------------------------------------------------------------------------------------------------------------
# 2. episodes in lock step with the host simulators
# ---------------------------------------------------------------------------------------------------------------------
def host_flags(info):
    viol = info.get("num_safety_violation", info.get("num_safety_violation_obstacles", 0))
    return int(bool(info.get("goal_met", False))), int(viol)


@pytest.mark.parametrize("name", TASKS)
def test_episodes_in_lock_step(name):
    iters, limit = 40, 15                                            # every lane reaches the time limit at 15 and 30
    env = D.make(name, N, SEED, device_resets=True, init_spread=SPREAD)
    env.max_episode_steps = limit
    hosts, obs = host_at(name, env.reset_noise.cpu().numpy())
    for h in hosts:
        h.max_episode_steps = limit
    np.testing.assert_allclose(env.obs.cpu().numpy(), obs, **TOL)
    table = actions(np.random.RandomState(9), env, iters)            # the fixed action table, (iters, N, 2)
    resets = np.zeros(N, dtype=np.int64)
    n_viol = 0
    for it in range(iters):
        env.step(torch.from_numpy(table[it]).cuda())
        outs = [h.step(table[it, i]) for i, h in enumerate(hosts)]
        done = np.array([int(bool(o[-2])) for o in outs], dtype=np.int32)
        goal, viol = (np.array(v) for v in zip(*[host_flags(o[-1]) for o in outs]))
        np.testing.assert_allclose(env.obs.cpu().numpy(), np.array([o[0] for o in outs]), err_msg="obs at step %d" % it, **TOL)
        # (Unicycle's first reward of an episode starts from the reset's last_dist)
        np.testing.assert_allclose(env.reward.cpu().numpy(), np.array([o[1] for o in outs]), err_msg="reward at step %d" % it, **TOL)
        assert np.array_equal(env.done.cpu().numpy(), done), "done at step %d" % it
        assert np.array_equal(env.info[:, 0].cpu().numpy(), goal.astype(np.float64)), "goal at step %d" % it
        assert np.array_equal(env.info[:, 1].cpu().numpy(), viol.astype(np.float64)), "violations at step %d" % it
        assert np.array_equal(env.ep_step.cpu().numpy(), np.array([h.episode_step for h in hosts]))
        n_viol += int(viol.sum())
        o32 = env.reset_done(env.done)
        offs = env.reset_noise.cpu().numpy()
        for i in np.flatnonzero(done):
            hosts[i].reset(offset=offs[i])
        resets += done
        fin = done > 0
        if fin.any():
            np.testing.assert_allclose(env.obs.cpu().numpy()[fin], np.array([h.get_obs() for h in hosts])[fin], **TOL)
            assert np.array_equal(env.state.cpu().numpy()[fin], np.array([h.state for h in hosts])[fin])
        assert torch.equal(o32, env.obs.to(torch.float32))
    print("%s: resets per lane %d - %d, safety violations %d" % (name, resets.min(), resets.max(), n_viol))
    assert resets.min() >= 2
    assert np.array_equal(env.reset_count.cpu().numpy(), resets + 1)                 # (+ the constructor's)


# ---------------------------------------------------------------------------------------------------------------------
# 3. no spread: nothing changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TASKS)
def test_no_spread_is_the_fixed_start(name, monkeypatch):
    seen, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (seen.append(fn), real(fn, *a))[1])
    zero = D.make(name, N, SEED, device_resets=True, init_spread=(0, 0))
    plain = D.make(name, N, SEED, device_resets=True)
    assert zero.init_spread == plain.init_spread == (0.0, 0.0)
    for e in (zero, plain):
        e.max_episode_steps = 25
    rs = np.random.RandomState(1)
    for _ in range(60):
        a = actions(rs, zero)
        for e in (zero, plain):
            e.step(a)
            e.reset_done()
    torch.cuda.synchronize()
    step = "nlbac_%s_env_step" % base(name).lower()
    assert set(seen) == {"nlbac_env_reset_rows", step} and not set(seen) & set(NEW)
    assert seen.count("nlbac_env_reset_rows") == 2 * (60 + 1) and seen.count(step) == 2 * 60   # (+ the constructor's reset)
    for key in list(float64_tensors(zero)) + ["ep_step", "reset_count", "obs32", "done"]:
        assert torch.equal(getattr(zero, key), getattr(plain, key)), key
    assert int(zero.reset_count.min()) == 3 and not bool(zero.reset_noise.any())
    ref = D.make(name, 1, SEED)                                       # host mode: the torch formulas of the fixed start
    zero.reset()
    assert torch.equal(zero.state, ref.state.expand(N, -1)) and torch.equal(zero.obs, ref.obs.expand(N, -1))


# ---------------------------------------------------------------------------------------------------------------------
# 4. evaluation: N lanes are N different episodes
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluation_of_distinct_episodes():
    n = 64
    agent, _ = make_agent(64, 64, 0, "euler", "Unicycle", 50.0)

    def returns(**kw):
        env = D.make("Unicycle", n, seed=0, device_resets=True, **kw)
        env.max_episode_steps = 40
        res = evaluate_vectorized(agent, env)
        assert res["episodes"] == n == len(res["history"]) and sorted(res["arrays"]["lane"]) == list(range(n))
        assert np.isfinite(res["arrays"]["reward"]).all() and (res["arrays"]["length"] <= 40).all()
        return res["arrays"]["reward"]
    spread, fixed = returns(init_spread=(0.3, 0.3)), returns(init_spread=(0, 0))
    print("returns with a spread: %d distinct of %d (std %.4f); without: %d distinct"
          % (len(np.unique(spread)), n, spread.std(), len(np.unique(fixed))))
    assert len(np.unique(spread)) > 1, "a start spread, and every lane ran the same episode"
    assert len(np.unique(fixed)) == 1, "the fixed start: one episode, n times"
    assert np.array_equal(fixed, returns())
