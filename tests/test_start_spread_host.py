"""Host-side checks of the start spread of the Unicycle and Pvtol simulators (``envs/device.py`` ``init_spread=``,
``csrc/env_reset_kernels.hip`` ``nlbac_unicycle_env_reset`` / ``nlbac_pvtol_env_reset``): the argument checks, which
refuse before the device is touched; ``reset(offset=)`` of the host simulators, the reference the kernels are held
against; the numpy restatement of the draw (``start_reset_offsets`` below — the GPU tests import it); the two entry
points' declarations and refusals; and the command line."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from nlbac_amd import envs, train
from nlbac_amd.envs import device as D
from nlbac_amd.synth import _pvtol_obs, _unicycle_obs
from test_env_reset_host import philox4x32_10
from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)

TASKS = ("Unicycle", "UnicycleBarrier", "Pvtol", "PvtolBarrier")
START = {"Unicycle": np.array([-2.5, -2.5]), "Pvtol": np.array([-4.5, -4.5])}
NAMES = ("nlbac_unicycle_env_reset", "nlbac_pvtol_env_reset")


def base(name):
    return name[:-len("Barrier")] if name.endswith("Barrier") else name


def start_reset_offsets(seed, lane, count, sx, sy):
    """The start-position offsets (dx, dy) of lane ``lane``'s reset number ``count`` under ``seed`` (csrc/philox.h has
    the definition): Philox counter (lane, count, 0, 4), two 52-bit uniforms, uniform on [-sx, sx] x [-sy, sy];
    float64, arrays broadcast, (k, 2) out."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x, y, z, w = (v.astype(np.uint64) for v in philox4x32_10((lane, count, 0, 4), (seed & 0xFFFFFFFF, seed >> 32)))
    m0 = (x << np.uint64(20)) | (y >> np.uint64(12))
    m1 = (z << np.uint64(20)) | (w >> np.uint64(12))
    u0 = (m0.astype(np.float64) + 0.5) * 2.0 ** -52
    u1 = (m1.astype(np.float64) + 0.5) * 2.0 ** -52
    return np.stack([sx * (2.0 * u0 - 1.0), sy * (2.0 * u1 - 1.0)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. arguments (every refusal comes before the device is touched: no GPU here)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TASKS)
def test_argument_checks(name):
    for bad in ((-0.1, 0.1), (0.1, -0.1), (np.nan, 0.1), (0.1, np.inf), (0.1,), (0.1, 0.1, 0.1)):
        with pytest.raises(ValueError, match="init_spread"):
            D.make(name, 4, device_resets=True, init_spread=bad)
    with pytest.raises(ValueError, match="device_resets"):
        D.make(name, 4, init_spread=(0.3, 0.3))
    with pytest.raises(ValueError, match="device_resets"):
        D.make(name, 4, device_resets=False, init_spread=(0.0, 0.1))


def test_argument_checks_by_class():
    with pytest.raises(ValueError, match="device_resets"):
        D.DeviceUnicycleEnv(4, init_spread=(0.3, 0.1))
    with pytest.raises(ValueError, match="device_resets"):
        D.DevicePvtolEnv(4, init_spread=(0.3, 0.1))
    with pytest.raises(ValueError, match="init_spread"):
        D.DevicePvtolEnv(4, device_resets=True, init_spread=(-1.0, 0.0), safety_operator_follow=0.5)


def test_a_spread_that_reaches_a_hazard_or_the_goal_is_refused():
    # Unicycle: start (-2.5, -2.5), centre (-2.47, -2.5); the nearest hazard is (-1.5, -1.5), radius 0.5.  A corner of
    # the rectangle 0.42 from it; then a side 0.4 below it
    for name in ("Unicycle", "UnicycleBarrier"):
        with pytest.raises(ValueError, match="hazard"):
            D.make(name, 4, device_resets=True, init_spread=(0.7, 0.7))
        with pytest.raises(ValueError, match="hazard"):
            D.make(name, 4, device_resets=True, init_spread=(2.0, 0.6))
    # Pvtol: start (-4.5, -4.5); the obstacle (-4.5, 0) of radius 0.25 is straight above (the segment ends 0.2 below
    # its centre), (-2.5, -2.5) lies on the diagonal (the corner 0.14 from its centre)
    for name in ("Pvtol", "PvtolBarrier"):
        with pytest.raises(ValueError, match="hazard"):
            D.make(name, 4, device_resets=True, init_spread=(0.0, 4.3))
        with pytest.raises(ValueError, match="hazard"):
            D.make(name, 4, device_resets=True, init_spread=(1.9, 1.9))
    # the goal region.  In both tasks' geometry a rectangle around the start meets a hazard before it meets the goal,
    # so the check itself is called, without hazards: Unicycle's goal is 0.3 around (2.5, 2.5), Pvtol's 3.5 around
    # (4.5, 4.5)
    none = np.zeros((0, 2))
    with pytest.raises(ValueError, match="goal"):
        D._check_start_box(D.DeviceUnicycleEnv, ((-2.5, -2.5), (-2.47, -2.5)), (4.8, 4.8), none, 0.5, np.array([2.5, 2.5]), 0.3)
    D._check_start_box(D.DeviceUnicycleEnv, ((-2.5, -2.5), (-2.47, -2.5)), (4.7, 4.7), none, 0.5, np.array([2.5, 2.5]), 0.3)
    with pytest.raises(ValueError, match="goal"):
        D._check_start_box(D.DevicePvtolEnv, ((-4.5, -4.5),), (6.6, 6.6), none, 0.25, np.array([4.5, 4.5]), 3.5)
    D._check_start_box(D.DevicePvtolEnv, ((-4.5, -4.5),), (6.5, 6.5), none, 0.25, np.array([4.5, 4.5]), 3.5)


def test_the_rectangle_against_disc_test():
    hit = D._box_meets_disc
    assert hit((0, 0), (1, 1), (2, 0), 1.0) and not hit((0, 0), (1, 1), (2, 0), 0.999)        # a side: closed disc
    assert hit((0, 0), (1, 1), (2, 2), 1.4143) and not hit((0, 0), (1, 1), (2, 2), 1.4142)    # a corner: sqrt(2)
    assert hit((0, 0), (1, 1), (0.5, -0.5), 0.0)                                              # the centre inside
    assert hit((0, 0), (0, 0), (0.3, 0.4), 0.5) and not hit((0, 0), (0, 0), (0.3, 0.4), 0.4999)   # no spread: a point
    # the largest square spreads the two tasks admit, from their geometry: Unicycle's centre (-2.47, -2.5) against the
    # hazard at (-1.5, -1.5) of radius 0.5, Pvtol's start against the obstacle at (-2.5, -2.5) of radius 0.25
    free = lambda cls, pts, s, hz, r, goal, size: D._check_start_box(cls, pts, (s, s), hz, r, goal, size)
    u, p = D.DeviceUnicycleEnv, D.DevicePvtolEnv
    from nlbac_amd.envspec import PvtolSpec, UnicycleSpec
    us, ps = UnicycleSpec(), PvtolSpec()
    free(u, ((-2.5, -2.5), (-2.47, -2.5)), 0.6, us.hazards_locations, us.hazards_radius, us.goal_pos, u.goal_size)
    with pytest.raises(ValueError, match="hazard"):
        free(u, ((-2.5, -2.5), (-2.47, -2.5)), 0.65, us.hazards_locations, us.hazards_radius, us.goal_pos, u.goal_size)
    free(p, ((-4.5, -4.5),), 1.8, ps.hazard_locations, ps.hazards_radius, ps.goal_pos, p.goal_size)
    with pytest.raises(ValueError, match="hazard"):
        free(p, ((-4.5, -4.5),), 1.83, ps.hazard_locations, ps.hazards_radius, ps.goal_pos, p.goal_size)


def test_defaults():
    for cls in (D.DeviceUnicycleEnv, D.DevicePvtolEnv, D.DeviceQuadrotorLikeEnv):
        assert inspect.signature(cls.__init__).parameters["init_spread"].default == (0.0, 0.0)
        assert tuple(cls.init_spread) == (0.0, 0.0)
        for f in (cls.reset, cls.reset_done):
            assert inspect.signature(f).parameters["noise"].default is None
    assert "init_spread" not in inspect.signature(D.DeviceSimulatedCarsEnv.__init__).parameters
    assert D.DeviceUnicycleEnv.start_state == (-2.5, -2.5, 0.0) and D.DeviceUnicycleEnv.start_center == (-2.47, -2.5)
    assert D.DevicePvtolEnv.start_state == (-4.5, -4.5, 0.0, 0.0, 0.0, 1.0, -4.5)
    for cls in (envs.UnicycleEnv, envs.PvtolEnv, envs.QuadrotorLikeEnv):
        assert inspect.signature(cls.reset).parameters["offset"].default is None


# ---------------------------------------------------------------------------------------------------------------------
# 2. reset(offset=) of the host simulators
# ---------------------------------------------------------------------------------------------------------------------
def fields(e):
    out = dict(state=e.state.copy(), last=float(e.last_goal_dist), k=e.episode_step)
    if hasattr(e, "center"):
        out.update(center=e.center.copy(), next_center=e.next_center.copy())
    return out


@pytest.mark.parametrize("name", TASKS)
def test_host_reset_without_an_offset_is_as_before(name):
    e = envs.make(name, 0)
    for _ in range(3):
        e.step(np.array([1.0, 0.5]))
    o0, f0 = e.reset(), fields(e)
    for off in (None, (0.0, 0.0), np.zeros(2)):
        e.step(np.array([1.0, 0.5]))
        o, f = e.reset(offset=off), fields(e)
        assert o.tobytes() == o0.tobytes(), off
        for k in f0:
            assert np.asarray(f[k]).tobytes() == np.asarray(f0[k]).tobytes(), (k, off)
    assert f0["k"] == 0


@pytest.mark.parametrize("name", TASKS)
def test_host_reset_with_an_offset(name):
    e = envs.make(name, 0)
    e.reset()
    f0 = fields(e)
    off = np.array([0.21, -0.13])
    e.step(np.array([1.0, 0.5]))
    obs, f = e.reset(offset=off), fields(e)
    st0, st = f0["state"], f["state"]
    moved = np.flatnonzero(st != st0)
    if base(name) == "Unicycle":
        assert list(moved) == [0, 1]
        assert np.array_equal(st[:2], st0[:2] + off)
        assert np.array_equal(f["center"], f0["center"] + off) and np.array_equal(f["next_center"], f["center"])
        assert f["last"] == np.linalg.norm(e.goal_pos - f["next_center"])
        np.testing.assert_allclose(f["center"], st[:2] + e.l_p * np.array([np.cos(st[2]), np.sin(st[2])]), rtol=0, atol=1e-15)
        want = _unicycle_obs(st[None], e.goal_pos)[0]
    else:
        assert list(moved) == [0, 1, 6]
        assert np.array_equal(st[:2], st0[:2] + off) and st[6] == st0[6] + off[0] and st[6] == st[0]
        assert f["last"] == np.linalg.norm(e.goal_pos - st[:2])
        want = _pvtol_obs(st[None], e.goal_pos)[0]
    assert f["k"] == 0 and obs.tobytes() == want.tobytes() and obs.tobytes() == e.get_obs().tobytes()
    # the formulas of the device simulators' step_obs, written out: position, heading, compass, exp(-distance)
    rel = e.goal_pos - st[:2]
    compass = rel / (np.linalg.norm(rel) + 0.001)                 # (heading 0: the body frame is the world frame)
    tail = np.concatenate([compass, [np.exp(-np.linalg.norm(rel))]])
    np.testing.assert_allclose(obs[:4], [st[0], st[1], 1.0, 0.0], rtol=0, atol=0)
    np.testing.assert_allclose(obs[-3:], tail, rtol=1e-15, atol=0)
    if base(name) == "Pvtol":
        assert np.array_equal(obs[4:8], st[3:7])
    # an episode from the moved start is an episode: the first step's reward uses the moved last distance
    out = e.step(np.array([1.0, 0.5]))
    assert np.isfinite(out[1]) and e.episode_step == 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. the draw
# ---------------------------------------------------------------------------------------------------------------------
def test_the_draw():
    lanes = np.arange(4096)
    s = (0.3, 0.2)
    a = start_reset_offsets(7, lanes, 0, *s)
    assert a.shape == (4096, 2) and a.dtype == np.float64
    assert np.array_equal(a, start_reset_offsets(7, lanes, 0, *s))                      # deterministic
    assert np.array_equal(a[:64], start_reset_offsets(7, np.arange(64), 0, *s))          # no lane count in it
    assert np.array_equal(a[5], start_reset_offsets(7, 5, 0, *s)[0])
    for other in (start_reset_offsets(8, lanes, 0, *s), start_reset_offsets(7, lanes, 1, *s),
                  start_reset_offsets(7 + (1 << 32), lanes, 0, *s)):                    # seed, count, the key's high word
        assert not (other == a).any()
    assert (np.abs(a) <= np.array(s)).all() and np.abs(a[:, 0]).max() > 0.29 and np.abs(a[:, 1]).max() > 0.19
    assert len(np.unique(a[:, 0])) == 4096 and len(np.unique(a[:, 1])) == 4096
    # uniform on [-s, s]: mean 0 and std s / sqrt(3); five standard errors, s / sqrt(3 n) of the mean and, with the
    # uniform's kurtosis 9 / 5, std sqrt((9 / 5 - 1) / (4 n)) = std sqrt(0.2 / n) of the std
    for c in range(2):
        assert abs(a[:, c].mean()) < 5 * s[c] / np.sqrt(3 * 4096)
        assert abs(a[:, c].std() - s[c] / np.sqrt(3)) < 5 * s[c] / np.sqrt(3) * np.sqrt(0.2 / 4096)
    # the scale is a plain factor, and no spread draws nothing
    assert np.array_equal(start_reset_offsets(7, lanes, 0, 0.6, 0.4), 2.0 * a)
    assert not start_reset_offsets(7, lanes, 0, 0.0, 0.0).any()
    # the extremes of the 52-bit uniforms stay inside: u in (0, 1), so |2 u - 1| < 1
    for m in (0, 2 ** 52 - 1):
        u = (np.float64(m) + 0.5) * 2.0 ** -52
        assert abs(0.3 * (2.0 * u - 1.0)) <= 0.3
    # a tag of its own: not the Quadrotor-like task's draw (tag 3) at the same counters
    x3 = philox4x32_10((lanes, 0, 0, 3), (7, 0))[0]
    x4 = philox4x32_10((lanes, 0, 0, 4), (7, 0))[0]
    assert not (x3 == x4).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    philox = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "philox.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in header           # (additions only)
    assert re.search(r"#define PHILOX_TAG_START_RESET 4u\b", philox)


def reset_args(name, params):
    from nlbac_amd import _lib
    host = (C.c_double * 64)()                   # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    par = (C.c_double * len(params))(*params)
    kw = dict(n=4, done=p, seed=0, params=par, noise=p, state=p, ep_step=p)
    if name == "nlbac_unicycle_env_reset":
        kw["last_dist"] = p
    kw.update(obs=p, obs32=p, reset_count=p, reset_noise=p, s=None)
    assert len(kw) == len(_lib._PROTOS[name]), name
    return kw, (host, par)


PARAMS = {"nlbac_unicycle_env_reset": [-2.5, -2.5, 0.0, -2.47, -2.5, 2.5, 2.5, 0.3, 0.3],
          "nlbac_pvtol_env_reset": [-4.5, -4.5, 0.0, 0.0, 0.0, 1.0, -4.5, 4.5, 4.5, 0.3, 0.3]}


@pytest.mark.parametrize("name", NAMES)
def test_refuses_before_launching(lib, name):
    assert getattr(lib, name) is not None
    kw, keep = reset_args(name, PARAMS[name])
    assert "n >= 1" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "n >= 1" in refused(lib, name, dict(kw, n=-3), "n < 0")
    required = [k for k in kw if k not in ("n", "done", "seed", "noise", "s")]
    assert len(required) == (8 if "unicycle" in name else 7)
    for k in required:
        assert "null pointer" in refused(lib, name, dict(kw, **{k: None}), "a null %s" % k)
    for at in (-2, -1):
        bad = list(PARAMS[name])
        bad[at] = -0.1
        kw2, keep2 = reset_args(name, bad)
        assert "spread" in refused(lib, name, kw2, "a negative spread")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_command_line():
    a = train.get_args(["--env", "Unicycle", "--vector_envs", "8"])
    assert a.vector_init_spread is None and a.vector_device_resets is False
    assert train.vector_env_options("Unicycle", False, a.vector_init_spread) == dict(device_resets=False)
    assert train.vector_env_options("SimulatedCars", True, None) == dict(device_resets=True)
    b = train.get_args(["--env", "Pvtol", "--vector_envs", "8", "--vector_init_spread", "0.3", "0.2"])
    assert b.vector_init_spread == [0.3, 0.2] and b.vector_device_resets is False
    for env in TASKS + ("QuadrotorLike",):                        # implies resets on the device; passed through
        assert train.vector_env_options(env, False, b.vector_init_spread) == dict(device_resets=True, init_spread=(0.3, 0.2))
    with pytest.raises(ValueError, match="SimulatedCars"):
        train.vector_env_options("SimulatedCars", True, b.vector_init_spread)
    with pytest.raises(SystemExit):
        train.get_args(["--env", "Pvtol", "--vector_init_spread", "0.3"])
