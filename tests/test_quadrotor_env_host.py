"""CPU: the Quadrotor-like task's host simulator (``envs.QuadrotorLikeEnv``) and its wiring.  The reference holds no
code for this task, so the simulator is pinned to what the repository already had: ``synth.quadrotor_transitions``'
one-step model (the rows the agent tests use) and ``QuadrotorLikeSpec``'s constants.  The episode figures of
``test_constant_action_episodes`` follow from that model alone (float64, Euler, dt 0.02)."""
import os
import re

import numpy as np
import pytest
import torch

import nlbac_amd  # noqa: F401
from nlbac_amd import _lib, envs, synth
from nlbac_amd.envspec import QuadrotorLikeSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds(env):
    return float(env.action_space.low[0]), float(env.action_space.high[0]), env.MASS * env.G / 2.0


def _mask(env, episode_steps, done):
    """the drivers' rule (train.train)"""
    return 1 if episode_steps == env.max_episode_steps else float(not done)


def _episode(env, action):
    """run one episode from reset() under a constant action -> per-step records"""
    env.reset()
    rec = []
    while True:
        obs, reward, constraint, signal, lya_pre, lya_next, done, info = env.step(action)
        rec.append(dict(signal=signal, viol=info["num_safety_violation"], cost=info["safety_cost"], done=done,
                        goal=info.get("goal_met", False), state=env.state.copy()))
        assert len(rec) <= env.max_episode_steps
        if done:
            return rec


def test_step_returns_the_barrier_eight_tuple():
    env = envs.make("QuadrotorLike")
    assert isinstance(env, envs.QuadrotorLikeEnv) and isinstance(env, QuadrotorLikeSpec)
    obs0 = env.reset()
    assert obs0.dtype == np.float64 and np.array_equal(obs0, np.array(env.start_state)) and env.episode_step == 0
    assert np.array_equal(env.get_obs(), obs0)
    out = env.step([0.1, 0.12])
    assert len(out) == 8
    obs, reward, constraint, signal, lya_pre, lya_next, done, info = out
    assert np.array_equal(lya_pre, obs0) and np.array_equal(lya_next, obs) and np.array_equal(obs, env.state)
    assert reward == -constraint and signal == 0.0 and not done and "goal_met" not in info
    assert info["num_safety_violation"] == 0 and info["safety_cost"] == 0.0 and env.episode_step == 1
    off = env.reset(offset=(0.25, -0.05))
    assert np.array_equal(off, np.array([1.5 + 0.25, 0.0, 0.3 + -0.05, 0.0, 0.0, 0.0]))


def test_constant_action_episodes():
    env = envs.make("QuadrotorLike")
    lo, hi, hover = _bounds(env)
    assert env.max_episode_steps == 500

    rec = _episode(env, (hover, hover))                       # hovers in place until the time limit
    assert len(rec) == 500 and sum(r["viol"] for r in rec) == 0 and not rec[-1]["goal"]
    assert np.abs(rec[-1]["state"] - np.array(env.start_state)).max() <= 1e-12
    assert _mask(env, len(rec), rec[-1]["done"]) == 1

    rec = _episode(env, (hi, hi))                             # climbs out of the range, then out of the crash box
    viol = [k + 1 for k, r in enumerate(rec) if r["viol"]]
    assert len(rec) == 53 and sum(r["viol"] for r in rec) == 11 and viol == list(range(43, 54))
    assert all(r["signal"] == (env.D1 if r["viol"] else 0.0) for r in rec)          # none of them is a hit
    assert all(r["viol"] in (0, 1) for r in rec) and rec[-1]["state"][2] > env.crash_z[1]
    assert _mask(env, len(rec), rec[-1]["done"]) == 0.0 and not rec[-1]["goal"]

    rec = _episode(env, (lo, lo))                             # falls through the floor
    viol = [k + 1 for k, r in enumerate(rec) if r["viol"]]
    assert len(rec) == 37 and sum(r["viol"] for r in rec) == 19 and viol[0] == 19
    assert rec[-1]["state"][2] < env.crash_z[0] and _mask(env, len(rec), rec[-1]["done"]) == 0.0

    for action in ((lo, hi), (hi, lo)):                       # tilts over
        rec = _episode(env, action)
        assert len(rec) == 6 and sum(r["viol"] for r in rec) == 0
        assert abs(rec[-1]["state"][4]) > env.crash_theta and _mask(env, len(rec), rec[-1]["done"]) == 0.0


def test_one_step_is_synth_quadrotor_transitions():
    env = envs.make("QuadrotorLike")
    tr = synth.quadrotor_transitions(512, seed=1)
    checked = 0
    for i in range(512):
        env.reset()
        env.state = tr["obs"][i].copy()
        obs, reward, constraint, signal, lya_pre, lya_next, done, info = env.step(tr["action"][i])
        np.testing.assert_allclose(obs, tr["next_obs"][i], rtol=1e-12, atol=0)
        np.testing.assert_allclose(constraint, tr["constraint"][i], rtol=1e-12, atol=0)
        np.testing.assert_allclose(signal, tr["barrier_signal"][i], rtol=1e-12, atol=0)
        assert np.array_equal(lya_pre, tr["obs"][i])
        if tr["constraint"][i] != 0.05:
            np.testing.assert_allclose(reward, tr["reward"][i], rtol=1e-12, atol=0)
            checked += 1
    assert checked >= 500
    assert set(np.unique(tr["barrier_signal"])) >= {0.0, env.D1, env.D2}             # the rows do exercise both signals


def test_hit_and_out_of_range():
    env = envs.make("QuadrotorLike")
    _, _, hover = _bounds(env)
    env.reset()
    env.state = np.array([env.obstacle[0] + 0.1, 0.0, env.obstacle[1], 0.0, 0.0, 0.0])
    *_, signal, _, _, done, info = env.step((hover, hover))
    assert signal == env.D2 and info["num_safety_violation"] == 1 and not done
    assert info["safety_cost"] == pytest.approx((0.25 - 0.1) / 0.25, rel=1e-9)
    env.reset()
    env.state = np.array([2.1, 0.0, 0.6, 0.0, 0.0, 0.0])       # out of the range alone: the episode goes on
    *_, signal, _, _, done, info = env.step((hover, hover))
    assert signal == env.D1 and info["num_safety_violation"] == 1 and not done
    assert info["safety_cost"] == pytest.approx(0.1, rel=1e-9)


def test_a_scripted_controller_reaches_the_goal_without_a_violation():
    """outer loop: PD on position (1.5 / 1.2 in x, 4 / 3 in z), desired tilt ax / G clipped to +-0.3; inner loop: tilt
    PD (60 / 12); thrusts clipped to the action bounds"""
    env = envs.make("QuadrotorLike")
    lo, hi, _ = _bounds(env)
    obs = env.reset()
    violations, steps, goal = 0, 0, False
    while steps < 200:
        x, vx, z, vz, th, om = obs
        ax = 1.5 * (env.goal_pos[0] - x) - 1.2 * vx
        az = 4.0 * (env.goal_pos[1] - z) - 3.0 * vz
        th_des = np.clip(ax / env.G, -0.3, 0.3)
        thrust = env.MASS * (env.G + az) / max(np.cos(th), 0.5)
        torque = env.IYY * (60.0 * (th_des - th) - 12.0 * om)
        diff = torque * np.sqrt(2.0) / env.ARM                 # a1 - a0
        action = np.clip([(thrust - diff) / 2.0, (thrust + diff) / 2.0], lo, hi)
        obs, _, _, _, _, _, done, info = env.step(action)
        steps += 1
        violations += info["num_safety_violation"]
        if done:
            goal = bool(info.get("goal_met", False))
            break
    assert goal and steps <= 200 and violations == 0, (goal, steps, violations)


def test_wiring():
    from nlbac_amd import train
    from nlbac_amd.envs import device as device_envs
    from nlbac_amd.sac_cbf_clf.dynamics import DynamicsModel
    args = train.get_args(["--env", "QuadrotorLike"])
    assert args.env == "QuadrotorLike" and train.has_barrier_signal(args.env)
    assert train.has_barrier_signal("UnicycleBarrier") and train.has_barrier_signal("PvtolBarrier")
    assert not any(train.has_barrier_signal(e) for e in ("Unicycle", "SimulatedCars", "Pvtol"))

    dm = DynamicsModel(envs.make("QuadrotorLike"), args)
    one, many = np.arange(6.0), np.arange(18.0).reshape(3, 6)
    for o in (one, many):
        s = dm.get_state(o)
        assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == o.shape and np.array_equal(s, o)
        assert s is not o
        t = torch.tensor(o, dtype=torch.float32)
        st = dm.get_state(t)
        assert torch.is_tensor(st) and st.dtype == torch.float32 and st.shape == t.shape and torch.equal(st, t)

    header = open(os.path.join(ROOT, "include", "nlbac_hip.h")).read()
    for name in ("nlbac_quadrotor_env_step", "nlbac_quadrotor_env_reset"):
        assert name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, header)
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in header       # (additions only)

    # a start spread is drawn by the reset launch: asking for one in host mode is refused before the device is touched
    with pytest.raises(ValueError, match="device_resets"):
        device_envs.DeviceQuadrotorLikeEnv(4, init_spread=(0.3, 0.1))
    with pytest.raises(ValueError, match="device_resets"):
        device_envs.make("QuadrotorLike", 4, init_spread=(0.0, 0.1))
    with pytest.raises(ValueError, match="init_spread"):
        device_envs.make("QuadrotorLike", 4, device_resets=True, init_spread=(-0.1, 0.1))


def test_spec_constants_stay():
    """no existing attribute moved (agent goldens and the oracle rest on them); the simulator's own are additions"""
    env = QuadrotorLikeSpec()
    assert (env.dt, env.max_episode_steps, env.D1, env.D2, env.obstacle_radius) == (0.02, 500, -1.0, -10.0, 0.25)
    assert (env.MASS, env.IYY, env.ARM, env.G) == (0.027, 1.4e-5, 0.0397, 9.8)
    assert list(env.goal_pos) == [0.0, 1.0] and list(env.obstacle) == [0.6, 0.6]
    assert env.x_range == (-2.0, 2.0) and env.z_range == (0.0, 2.0)
    assert tuple(env.start_state) == (1.5, 0, 0.3, 0, 0, 0) and (env.goal_size, env.reward_goal) == (0.05, 250.0)
    assert env.crash_x == (-3, 3) and env.crash_z == (-1, 3) and env.crash_theta == np.pi / 2
    assert tuple(env.init_spread) == (0.0, 0.0)
    # the straight line from the start to the goal passes within 0.11 of the obstacle's centre
    p, g, c = np.array([1.5, 0.3]), np.array(env.goal_pos), np.array(env.obstacle)
    d = g - p
    assert abs(d[0] * (c - p)[1] - d[1] * (c - p)[0]) / np.linalg.norm(d) < 0.11 < env.obstacle_radius
