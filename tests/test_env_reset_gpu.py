"""GPU: the simulators' resets on the device (``envs/device.py`` ``device_resets=True``, ``csrc/env_reset_kernels.hip``)
against the host-mode resets (torch ops, numpy draws), lane by lane: a reset lane holds the host mode's bits, a lane that
goes on keeps every float64 value the step kernel wrote, ``obs32`` is the float32 observation of every lane, and the
SimulatedCars draw is the counter-based one ``tests/test_env_reset_host.py`` restates in numpy."""
import os

import numpy as np
import pytest
import torch

from nlbac_amd.envs import device as D
from oracle.gen_driver_golden import ScriptedAgent
from test_env_reset_host import cars_reset_offset

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = dict(rtol=1e-9, atol=1e-11)          # the simulators' tolerance in tests/test_device_envs_gpu.py


def flags(mask):
    return torch.as_tensor(np.asarray(mask).astype(np.int32), device="cuda")


def scripted_masks(rs, n):
    """none, all, a random third, lane 0 only, lane 255 only, lane 256 only, the last lane only; cycled"""
    def only(i):
        m = np.zeros(n, dtype=bool)
        m[i] = True
        return m
    k = 0
    while True:
        yield [np.zeros(n, dtype=bool), np.ones(n, dtype=bool), rs.rand(n) < 1.0 / 3.0, only(0), only(255), only(256),
               only(n - 1)][k % 7]
        k += 1


def actions(rs, env):
    lo, hi = np.asarray(env.action_space.low, dtype=np.float64), np.asarray(env.action_space.high, dtype=np.float64)
    return rs.uniform(lo, hi, size=(env.n, env.act_dim))


# ---------------------------------------------------------------------------------------------------------------------
# 1. device mode against host mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Unicycle", "UnicycleBarrier", "Pvtol", "PvtolBarrier"])
def test_device_mode_against_host_mode(name):
    N = 600                                  # workgroups of 256, 256, 88 lanes
    host, dev = D.make(name, N, 0), D.make(name, N, 0, device_resets=True)
    assert host.device_resets is False and dev.device_resets is True
    assert not hasattr(host, "obs32") and not hasattr(host, "reset_count")
    assert dev.obs32.dtype == torch.float32 and dev.reset_count.dtype == torch.int32
    rs = np.random.RandomState(11)
    masks = scripted_masks(np.random.RandomState(12), N)
    count = np.ones(N, dtype=np.int64)       # the construction's one
    worst = 0.0
    for k in range(30):
        a = actions(rs, host)
        host.step(a)
        dev.step(a)
        mask = next(masks)
        count += mask
        m = torch.as_tensor(mask, device="cuda")
        before = dev.obs.clone()
        o_host, o_dev = host.reset_done(flags(mask)), dev.reset_done(flags(mask))
        assert o_dev is dev.obs32 and o_host.dtype == torch.float32
        assert torch.equal(o_host, host.obs.to(torch.float32))
        assert torch.equal(dev.state, host.state) and torch.equal(dev.ep_step, host.ep_step)
        if hasattr(host, "last_dist"):
            assert torch.equal(dev.last_dist, host.last_dist)
        assert torch.equal(dev.obs[m], host.obs[m]), "a reset lane's observation differs from the host mode's"
        assert torch.equal(dev.obs[~m], before[~m]), "a lane that goes on lost the observation the step wrote"
        np.testing.assert_allclose(dev.obs[~m].cpu().numpy(), host.obs[~m].cpu().numpy(), **TOL)
        assert torch.equal(dev.obs32, dev.obs.to(torch.float32))
        assert np.array_equal(dev.reset_count.cpu().numpy(), count)
        worst = max(worst, float((dev.obs - host.obs).abs().max()))
    print("%s: largest |obs(device mode) - obs(host mode)| over 30 steps: %.3e" % (name, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 2. edges
# ---------------------------------------------------------------------------------------------------------------------
def tensors(env):
    names = ["state", "ep_step", "obs", "reset_count", "reward", "constraint", "signal", "lya_pre", "lya_next", "done",
             "info"] + [k for k in ("last_dist", "t", "reset_noise") if hasattr(env, k)]
    return {k: getattr(env, k) for k in names}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536])
@pytest.mark.parametrize("name", ["Unicycle", "Pvtol", "SimulatedCars"])
def test_edges(name, n):
    env = D.make(name, n, 0, device_resets=True)
    start_state, start_obs = env.state.clone(), env.obs.clone()      # (the construction's reset: every lane at its start)
    if name != "SimulatedCars":
        ref = D.make(name, 1, 0)                                     # host mode: the torch formulas
        assert torch.equal(start_state, ref.state.expand(n, -1)) and torch.equal(start_obs, ref.obs.expand(n, -1))
    rs = np.random.RandomState(n % 1000)
    for _ in range(3):
        env.step(actions(rs, env))
    mask = rs.rand(n) < 0.5
    if n == 1:
        mask[:] = True
    m = torch.as_tensor(mask, device="cuda")
    before = {k: v.clone() for k, v in tensors(env).items()}
    out = env.reset_done(flags(mask))
    assert out is env.obs32 and torch.equal(env.obs32, env.obs.to(torch.float32))
    for k, v in tensors(env).items():
        assert torch.equal(v[~m], before[k][~m]), "%s of a lane that was not reset changed" % k
    assert bool((env.ep_step[m] == 0).all()) and bool((env.reset_count[m] == 2).all())
    if name == "SimulatedCars":
        pos = torch.tensor([42.0, 34.0, 26.0, 18.0, 10.0], dtype=torch.float64, device="cuda")
        assert torch.equal(env.state[m][:, ::2], pos.expand(int(m.sum()), -1))
        assert bool((env.state[m][:, 7] == 3.0).all()) and bool((env.t[m] == 0.0).all())
        for c in (1, 3, 5, 9):
            assert torch.equal(env.state[m][:, c], 3.0 + env.reset_noise[m])
        assert torch.equal(env.obs[m][:, ::2], env.state[m][:, ::2] / 100.0)
        assert torch.equal(env.obs[m][:, 1::2], env.state[m][:, 1::2] / 30.0)
    else:
        assert torch.equal(env.state[m], start_state[m]) and torch.equal(env.obs[m], start_obs[m])
        if hasattr(env, "last_dist"):
            assert bool((env.last_dist[m] == float(np.linalg.norm(env.goal_pos - np.array([-2.47, -2.5])))).all())
    # done=None is env.done: a run to the time limit resets every lane
    env.max_episode_steps = 3
    env.reset()
    for _ in range(3):
        env.step(actions(rs, env))
    assert bool((env.done == 1).all())
    count = env.reset_count.clone()
    env.reset_done()
    assert bool((env.ep_step == 0).all()) and torch.equal(env.reset_count, count + 1)
    assert torch.equal(env.obs32, env.obs.to(torch.float32))
    if name != "SimulatedCars":
        assert torch.equal(env.state, start_state) and torch.equal(env.obs, start_obs)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the cars draw
# ---------------------------------------------------------------------------------------------------------------------
def cars_run(n, seed, masks, twin=None, steps_between=0):
    """A device-mode cars environment taken through ``masks`` (None: a full ``reset()``), ``steps_between`` simulator
    steps before each; returns the environment, the offsets by (count, lane) (NaN where a lane never reached the
    count) and the largest difference from the numpy restatement.  ``twin``: a host-mode environment that is given
    every reset's offsets and must stay equal — in every bit while no step lies between the resets; with steps in
    between, a lane that goes on keeps the step kernel's observation in device mode while the host mode scales its
    state anew (torch's reciprocal product against the kernel's division), so those lanes' ``obs`` agree within the
    simulators' tolerance and everything else in every bit."""
    env = D.make("SimulatedCars", n, seed, device_resets=True)
    rs = np.random.RandomState(7)
    hist = np.full((len(masks) + 1, n), np.nan)
    count = np.zeros(n, dtype=np.int64)
    lanes = np.arange(n)
    worst = 0.0

    def took(mask):
        nonlocal worst
        got = env.reset_noise.cpu().numpy()
        want = cars_reset_offset(seed, lanes[mask], count[mask])
        worst = max(worst, float(np.abs(got[mask] - want).max()) if mask.any() else 0.0)
        hist[count[mask], lanes[mask]] = got[mask]
        count[mask] += 1
        assert np.array_equal(env.reset_count.cpu().numpy(), count)
        assert bool((env.state[torch.as_tensor(mask, device="cuda")][:, 7] == 3.0).all()), "car 4's velocity"
        if twin is not None:
            twin.reset(mask, noise=env.reset_noise.cpu())
            for k in ("state", "t", "ep_step"):
                assert torch.equal(getattr(env, k), getattr(twin, k)), k
            m = torch.as_tensor(mask, device="cuda")
            assert torch.equal(env.obs[m], twin.obs[m]), "a reset lane's observation differs from the host mode's"
            if steps_between == 0:
                assert torch.equal(env.obs, twin.obs)
            else:
                np.testing.assert_allclose(env.obs[~m].cpu().numpy(), twin.obs[~m].cpu().numpy(), **TOL)

    took(np.ones(n, dtype=bool))                                     # the constructor's reset
    for mask in masks:
        for _ in range(steps_between):
            a = actions(rs, env)
            env.step(a)
            if twin is not None:
                twin.step(a)
        prev = env.reset_noise.clone()
        if mask is None:
            env.reset()
            mask = np.ones(n, dtype=bool)
        else:
            env.reset_done(flags(mask))
        keep = torch.as_tensor(~mask, device="cuda")
        assert torch.equal(env.reset_noise[keep], prev[keep])
        took(mask)
    return env, hist, worst


def test_the_cars_draw():
    N = 600
    twin = D.make("SimulatedCars", N, 0)                             # (host mode: its constructor seeds and draws)
    state = np.random.get_state()
    rm = np.random.RandomState(21)
    masks = [None, np.ones(N, dtype=bool)] + [rm.rand(N) < 0.4 for _ in range(3)]
    env, hist, worst = cars_run(N, 0, masks, twin=twin)
    print("largest |reset_noise - numpy restatement|: %.3e" % worst)
    assert worst <= 1e-12
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:], \
        "numpy's global generator moved"
    # a lane's k-th offset does not depend on the lane count ...
    _, hist70, worst70 = cars_run(70, 0, [None if m is None else m[:70] for m in masks])
    assert worst70 <= 1e-12 and np.array_equal(hist70, hist[:, :70], equal_nan=True)
    # ... nor on when its k-th reset happened: other masks, other numbers of steps in between
    other = [rm.rand(N) < 0.7 for _ in range(4)] + [None]
    twin2 = D.make("SimulatedCars", N, 0)
    np.random.set_state(state)                                       # (the twin's constructor seeded and drew)
    _, hist2, worst2 = cars_run(N, 0, other, twin=twin2, steps_between=2)
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:], "numpy's global generator moved"
    both = ~np.isnan(hist) & ~np.isnan(hist2)
    assert worst2 <= 1e-12 and both[2:].sum() > N and np.array_equal(hist[both], hist2[both])
    # another seed, other draws
    _, hist3, worst3 = cars_run(N, 3, [None])
    assert worst3 <= 1e-12 and not np.any(hist3[:2] == hist[:2])
    assert np.nanmax(np.abs(hist)) < 3.0


def test_the_cars_draw_statistics():
    """65536 lanes, count 0: five standard errors of the mean (0.5 / sqrt(n)) and of the std (0.5 / sqrt(2 n))."""
    env = D.make("SimulatedCars", 65536, 0, device_resets=True)
    off = env.reset_noise.cpu().numpy()
    print("mean %.5f std %.5f" % (off.mean(), off.std()))
    assert abs(off.mean()) <= 0.01 and abs(off.std() - 0.5) <= 0.007
    assert np.abs(off - cars_reset_offset(0, np.arange(65536), 0)).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reference's trace through the device reset
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_trace_through_the_device_reset():
    """tests/test_device_envs_gpu.py::test_device_env_reproduces_the_reference_trace[SimulatedCars] with every reset a
    ``reset_done(all lanes, noise=the trace's draw)`` of a device-mode environment."""
    name, N = "SimulatedCars", 3
    g = np.load(os.path.join(GOLD, "driver_%s.npz" % name))
    env = D.make(name, N, 0, device_resets=True)
    env.max_episode_steps = int(g["meta_max_steps"])
    agent = ScriptedAgent(name, env.action_space, pattern=int(g["meta_pattern"]))
    n, backup = len(g["reward"]), g["backup"]
    every = torch.ones(N, dtype=torch.int32, device="cuda")
    state = np.random.get_state()
    try:
        np.random.seed(0)
        np.random.normal(0, 0.5)             # (the reference env's constructor takes the first draw)

        def reset():
            o32 = env.reset_done(every, noise=[np.random.normal(0, 0.5)] * N)
            assert torch.equal(o32, env.obs.to(torch.float32))
        reset()
        kept = []                            # (every step's outputs stay on the device: one copy at the end)
        for k in range(n):
            a = agent.select_action_backup(None) if backup[k] else agent.select_action(None)
            out = env.step(np.tile(a, (N, 1)))
            obs, reward, constraint = out[:3]
            lya, nlya, done, info = out[-4:]
            kept.append(torch.cat([obs.reshape(-1), reward[:1], constraint[:1], lya[1], nlya[2], done[:1].double(),
                                   info["num_safety_violation"][:1], info["safety_cost"][:1], info["reached"][:1]]))
            if g["done"][k]:
                reset()
        got = torch.stack(kept).cpu().numpy()
        at = np.cumsum([0, 10 * N, 1, 1, 4, 4, 1, 1, 1, 1])
        obs, reward, constraint, lya, nlya, done, n_viol, cost, reached = (got[:, at[j]:at[j + 1]] for j in range(9))
        for e in range(N):                   # every copy, advanced by the same launch
            np.testing.assert_allclose(obs[:, 10 * e:10 * e + 10], g["obs"], **TOL)
        np.testing.assert_allclose(reward[:, 0], g["reward"], **TOL)
        np.testing.assert_allclose(constraint[:, 0], g["constraint"], **TOL)
        np.testing.assert_allclose(lya, g["lya"], **TOL)
        np.testing.assert_allclose(nlya, g["next_lya"], **TOL)
        assert np.array_equal(done[:, 0].astype(bool), g["done"].astype(bool))
        assert np.array_equal(n_viol[:, 0], g["n_violation"])
        np.testing.assert_allclose(cost[:, 0], g["safety_cost"], rtol=1e-8, atol=1e-11)
        assert np.array_equal(reached[:, 0], g["reached"])
    finally:
        np.random.set_state(state)
