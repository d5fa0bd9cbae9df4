"""Batched simulators on the device: ``n_envs`` independent copies of a reference environment,
advanced by ONE launch per step (``csrc/env_kernels.hip``, float64 like the reference's numpy simulators).  Same
``reset`` / ``step`` contract as the host simulators of ``nlbac_amd.envs`` with a leading batch axis and device tensors:

    obs, reward, constraint[, barrier_signal], lya_in, next_lya_in, done, info = env.step(action)   # action (n, n_u)

``info`` is a dict of (n,) tensors (``goal_met`` / ``reached``, ``num_safety_violation``, ``safety_cost``).  Finished
environments are NOT reset behind the caller's back: ``reset(mask)`` resets those selected (``done`` of the last step
by default), so the terminal observation is what ``step`` returned — the reference driver's semantics.

``reset_done(done)`` is what a vectorised driver calls after every step: it resets the finished lanes and returns the
float32 observation the policy reads next.  With ``device_resets=False`` (the default) that is ``reset(done > 0)`` and a
float32 copy of ``obs``, torch ops with host syncs; with ``device_resets=True`` it is ONE launch
(``csrc/env_reset_kernels.hip``) and no host read, the lanes that go on keep the observation the step kernel wrote, and
SimulatedCars draws its initial-velocity offsets on the device from a counter-based generator ("Resets on
the device") instead of numpy's global one; Unicycle, Pvtol, their barrier copies and the Quadrotor-like task draw their
start positions the same way where an ``init_spread`` is asked for, so that N lanes are N different episodes.

Checked against traces recorded from the reference's own env classes (tests/test_device_envs_gpu.py); the Quadrotor-like
task, for which the reference holds no code, against the host simulator (tests/test_quadrotor_env_gpu.py); the drawn
starts against the host simulators' ``reset(offset=)`` (tests/test_start_spread_gpu.py).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..arena import stream_ptr
from ..envspec import PvtolSpec, QuadrotorLikeSpec, SimulatedCarsSpec, UnicycleSpec


def _dparams(*v):
    return (C.c_double * len(v))(*[float(x) for x in v])


class _DeviceEnv:
    state_dim = obs_dim = lya_dim = act_dim = 0

    def _common(self, n_envs, device):
        _lib.load()
        self.n, self.device = int(n_envs), torch.device(device)
        z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=self.device)
        self.state = z(self.n, self.state_dim)
        self.ep_step = z(self.n, dtype=torch.int32)
        self.obs, self.reward, self.constraint, self.signal = z(self.n, self.obs_dim), z(self.n), z(self.n), z(self.n)
        self.lya_pre, self.lya_next = z(self.n, self.lya_dim), z(self.n, self.lya_dim)
        self.done = z(self.n, dtype=torch.int32)
        self.info = z(self.n, 3)
        self._all = torch.ones(self.n, dtype=torch.bool, device=self.device)

    def _device_buffers(self):
        """device mode: the float32 observation every ``reset_done`` leaves and the per-lane reset counter"""
        self.obs32 = torch.zeros(self.n, self.obs_dim, dtype=torch.float32, device=self.device)
        self.reset_count = torch.zeros(self.n, dtype=torch.int32, device=self.device)

    def _flags(self, done):
        """``done`` as the launch reads it: None (every lane), or a contiguous int32 (n,) device tensor"""
        if done is None:
            return None
        d = torch.as_tensor(done, device=self.device)
        if d.dtype != torch.int32:
            d = d.to(torch.int32)                  # (a bool mask: one torch op)
        return d.reshape(self.n).contiguous()

    def _launch_reset(self, flags):
        """device mode: restart the lanes with ``flags > 0`` (None: every lane), refresh ``obs32``; one launch"""
        _lib.call("nlbac_env_reset_rows", self.n, None if flags is None else flags.data_ptr(), self.state_dim,
                  self.obs_dim, self._start_state.data_ptr(), self._start_obs.data_ptr(), float(self._start_last_dist),
                  self.state.data_ptr(), self.ep_step.data_ptr(),
                  self.last_dist.data_ptr() if getattr(self, "last_dist", None) is not None else None,
                  self.obs.data_ptr(), self.obs32.data_ptr(), self.reset_count.data_ptr(), stream_ptr())

    def _capture_start(self):
        """device mode, once at construction: the start rows, from the host-mode formulas (the torch ``reset`` on every
        lane), so that a reset lane's observation is the host mode's bit for bit"""
        self._host_reset(None)
        self._start_state = self.state[0].clone().contiguous()
        self._start_obs = self.obs[0].clone().contiguous()
        last = getattr(self, "last_dist", None)
        self._start_last_dist = float(last[0]) if last is not None else 0.0

    def reset(self, mask=None):
        if not self.device_resets:
            return self._host_reset(mask)
        self._launch_reset(None if mask is None else self._flags(torch.as_tensor(mask, device=self.device).bool()))
        return self.obs

    def reset_done(self, done=None):
        """Reset the lanes with ``done > 0`` (default: ``self.done``, the last step's) and return the float32
        ``(n, obs_dim)`` observation for the next step.  Host mode: ``reset(done > 0)`` and a fresh float32 copy of
        ``obs``.  Device mode: one launch and no host read; what is returned is ``self.obs32``, a PERSISTENT buffer that
        the next ``reset_done`` / ``reset`` overwrites — clone it to keep it.  ``done``: a contiguous int32 (n,) device
        tensor (the simulator's own ``done``), or a bool tensor, converted by one torch op."""
        done = self.done if done is None else done
        if not self.device_resets:
            d = torch.as_tensor(done, device=self.device)
            self.reset(d if d.dtype == torch.bool else d > 0)
            return self.obs.to(torch.float32).clone()
        self._launch_reset(self._flags(done))
        return self.obs32

    def _action(self, action):
        a = torch.as_tensor(action, device=self.device).to(torch.float64).reshape(self.n, self.act_dim).contiguous()
        return a

    def _info(self, first):
        return {first: self.info[:, 0], "num_safety_violation": self.info[:, 1], "safety_cost": self.info[:, 2]}


def _spread_of(cls, init_spread, device_resets):
    """``init_spread`` of the class ``cls`` as two floats, checked: finite, not negative, and drawn on the device only"""
    spread = tuple(float(v) for v in init_spread)
    if len(spread) != 2 or not all(np.isfinite(v) and v >= 0.0 for v in spread):
        raise ValueError("%s: init_spread is two finite non-negative floats (got %r)" % (cls.__name__, init_spread))
    if any(spread) and not device_resets:
        raise ValueError("%s: a start spread is drawn by the reset launch on the device: init_spread=%r needs "
                         "device_resets=True" % (cls.__name__, init_spread))
    return spread


def _box_meets_disc(centre, half, disc, radius):
    """the rectangle ``centre`` ± ``half`` against the closed disc ``radius`` around ``disc``: the distance from the
    disc's centre to the nearest point of the rectangle"""
    gap = np.maximum(np.abs(np.asarray(disc, dtype=np.float64) - np.asarray(centre, dtype=np.float64)) -
                     np.asarray(half, dtype=np.float64), 0.0)
    return float(np.hypot(gap[0], gap[1])) <= float(radius)


def _check_start_box(cls, points, spread, hazards, hazards_radius, goal_pos, goal_size):
    """No draw may start an episode inside a hazard or at the goal: nothing is rejected on the device, so a spread
    whose rectangle around one of ``points`` (the start position; for the Unicycle also the centre the hazards are
    tested against) reaches a hazard disc or the goal region is refused here."""
    for p in points:
        for h in np.asarray(hazards, dtype=np.float64):
            if _box_meets_disc(p, spread, h, hazards_radius):
                raise ValueError("%s: init_spread=%r reaches the hazard at (%g, %g), radius %g, from the start (%g, %g)"
                                 % (cls.__name__, tuple(spread), h[0], h[1], hazards_radius, p[0], p[1]))
        if _box_meets_disc(p, spread, goal_pos, goal_size):
            raise ValueError("%s: init_spread=%r reaches the goal region at (%g, %g), size %g, from the start (%g, %g)"
                             % (cls.__name__, tuple(spread), goal_pos[0], goal_pos[1], goal_size, p[0], p[1]))


class _StartSpread:
    """Start positions drawn per reset (``init_spread``) for a ``_DeviceEnv``: the draws are made by the reset's own
    launch from counters (seed, lane, reset number) and need ``device_resets=True``.  ``reset_noise`` (n, 2) holds every
    lane's last offsets, ``reset_count`` the number of its resets (the constructor's included).  Without a spread and
    without given offsets the reset is the generic ``nlbac_env_reset_rows``.  A class names its launch in
    ``_launch_spread_reset(flags pointer, offsets pointer)``."""

    def _spread_buffers(self, seed):
        self.reset_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.reset_noise = torch.zeros(self.n, 2, dtype=torch.float64, device=self.device)

    def _noise(self, noise):
        if noise is None:
            return None
        return torch.as_tensor(noise, dtype=torch.float64, device=self.device).reshape(self.n, 2).contiguous()

    def _launch_reset(self, flags, noise=None):
        if noise is None and not any(self.init_spread):
            return _DeviceEnv._launch_reset(self, flags)           # (the fixed start: the generic row reset)
        nz = self._noise(noise)
        self._launch_spread_reset(None if flags is None else flags.data_ptr(), None if nz is None else nz.data_ptr())

    def reset(self, mask=None, noise=None):
        """``noise``: (n, 2) start-position offsets to use in place of the lanes' draws (device mode only)."""
        if not self.device_resets:
            if noise is not None:
                raise ValueError("%s.reset: start offsets need device_resets=True" % type(self).__name__)
            return self._host_reset(mask)
        self._launch_reset(None if mask is None else self._flags(torch.as_tensor(mask, device=self.device).bool()), noise)
        return self.obs

    def reset_done(self, done=None, noise=None):
        """``_DeviceEnv.reset_done``; ``noise``: as for ``reset``."""
        if not self.device_resets:
            if noise is not None:
                raise ValueError("%s.reset_done: start offsets need device_resets=True" % type(self).__name__)
            return _DeviceEnv.reset_done(self, done)
        self._launch_reset(self._flags(self.done if done is None else done), noise)
        return self.obs32


class DeviceUnicycleEnv(_StartSpread, UnicycleSpec, _DeviceEnv):
    """U/envs/unicycle_env.py:57-152 for ``n_envs`` environments (``barrier=True``: NU's barrier signal as well).

    ``init_spread=(sx, sy)``: every reset draws its start position, x = -2.5 + sx (2 u0 - 1), y = -2.5 + sy (2 u1 - 1),
    so that N lanes are N different episodes (``_StartSpread``; one launch, ``nlbac_unicycle_env_reset``).  The centre
    ``l_p`` ahead of the position moves with it, and ``last_dist`` starts from the moved centre's distance to the goal;
    the heading stays 0.  A spread that reaches a hazard disc or the goal region is refused."""
    state_dim, obs_dim, lya_dim, act_dim = 3, 7, 2, 2
    reward_goal, goal_size, l_p = 500.0, 0.3, 0.03
    little_b, capital_b = 0.0, -20.0
    start_state, start_center = (-2.5, -2.5, 0.0), (-2.47, -2.5)
    init_spread = (0.0, 0.0)

    def __init__(self, n_envs, seed=0, barrier=False, device="cuda", device_resets=False, init_spread=(0.0, 0.0)):
        spread = _spread_of(type(self), init_spread, device_resets)
        UnicycleSpec.__init__(self, seed)
        if any(spread):
            _check_start_box(type(self), (self.start_state[:2], self.start_center), spread, self.hazards_locations,
                             self.hazards_radius, self.goal_pos, self.goal_size)
        self.barrier, self.device_resets, self.init_spread = barrier, bool(device_resets), spread
        self._common(n_envs, device)
        self.last_dist = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self._hz = torch.tensor(np.asarray(self.hazards_locations), dtype=torch.float64, device=self.device).contiguous()
        if self.device_resets:
            self._device_buffers()
            self._capture_start()
            self._spread_buffers(seed)
            self._reset_par = _dparams(*(self.start_state + self.start_center + tuple(self.goal_pos) + spread))
        self.reset()

    def _launch_spread_reset(self, flags, noise):
        _lib.call("nlbac_unicycle_env_reset", self.n, flags, self.reset_seed, self._reset_par, noise,
                  self.state.data_ptr(), self.ep_step.data_ptr(), self.last_dist.data_ptr(), self.obs.data_ptr(),
                  self.obs32.data_ptr(), self.reset_count.data_ptr(), self.reset_noise.data_ptr(), stream_ptr())

    def _host_reset(self, mask=None):
        m = self._all if mask is None else torch.as_tensor(mask, device=self.device).bool()
        self.state[m] = torch.tensor([-2.5, -2.5, 0.0], dtype=torch.float64, device=self.device)
        self.ep_step[m] = 0
        self.last_dist[m] = float(np.linalg.norm(self.goal_pos - np.array([-2.47, -2.5])))
        self.step_obs()
        return self.obs

    def step_obs(self):
        """observation of the current states (what ``reset`` returns)"""
        st = self.state
        rx, ry = self.goal_pos[0] - st[:, 0], self.goal_pos[1] - st[:, 1]
        c, s = torch.cos(st[:, 2]), torch.sin(st[:, 2])
        v0, v1 = rx * c + ry * s, -rx * s + ry * c
        n = torch.sqrt(v0 * v0 + v1 * v1) + 0.001
        self.obs.copy_(torch.stack([st[:, 0], st[:, 1], c, s, v0 / n, v1 / n, torch.exp(-torch.sqrt(rx * rx + ry * ry))], 1))

    def step(self, action):
        a = self._action(action)
        par = _dparams(self.dt, self.goal_pos[0], self.goal_pos[1], self.goal_size, self.reward_goal, self.hazards_radius,
                       self.l_p, self.little_b, self.capital_b)
        _lib.call("nlbac_unicycle_env_step", self.n, par, int(self.max_episode_steps), self._hz.data_ptr(),
                  self._hz.shape[0], a.data_ptr(), self.state.data_ptr(), self.ep_step.data_ptr(),
                  self.last_dist.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.constraint.data_ptr(),
                  self.signal.data_ptr(), self.lya_pre.data_ptr(), self.lya_next.data_ptr(), self.done.data_ptr(),
                  self.info.data_ptr(), stream_ptr())
        out = (self.obs, self.reward, self.constraint) + ((self.signal,) if self.barrier else ())
        return out + (self.lya_pre, self.lya_next, self.done, self._info("goal_met"))


class DevicePvtolEnv(_StartSpread, PvtolSpec, _DeviceEnv):
    """P/envs/pvtol_env.py:85-216 for ``n_envs`` environments (``barrier=True``: NP's barrier signal as well); the
    Lyapunov inputs are the observations before / after the step.

    ``init_spread=(sx, sy)``: every reset draws its start position, x = -4.5 + sx (2 u0 - 1), y = -4.5 + sy (2 u1 - 1),
    so that N lanes are N different episodes (``_StartSpread``; one launch, ``nlbac_pvtol_env_reset``; ``_host_reset``
    says which state components move).  A spread that reaches an obstacle's disc or the goal region is refused."""
    state_dim, obs_dim, lya_dim, act_dim = 7, 11, 11, 2
    reward_goal, goal_size = 1500.0, 3.5
    little_b, capital_b = 0.0, -0.1
    start_state = (-4.5, -4.5, 0.0, 0.0, 0.0, 1.0, -4.5)
    init_spread = (0.0, 0.0)

    def __init__(self, n_envs, seed=0, barrier=False, device="cuda", device_resets=False, init_spread=(0.0, 0.0),
                 **overrides):
        spread = _spread_of(type(self), init_spread, device_resets)
        PvtolSpec.__init__(self, seed, **overrides)
        if any(spread):
            _check_start_box(type(self), (self.start_state[:2],), spread, self.hazard_locations, self.hazards_radius,
                             self.goal_pos, self.goal_size)
        self.barrier, self.device_resets, self.init_spread = barrier, bool(device_resets), spread
        self._common(n_envs, device)
        self._hz = torch.tensor(np.asarray(self.hazard_locations), dtype=torch.float64, device=self.device).contiguous()
        if self.device_resets:
            self._device_buffers()
            self._capture_start()
            self._spread_buffers(seed)
            self._reset_par = _dparams(*(self.start_state + tuple(self.goal_pos) + spread))
        self.reset()

    def _launch_spread_reset(self, flags, noise):
        _lib.call("nlbac_pvtol_env_reset", self.n, flags, self.reset_seed, self._reset_par, noise, self.state.data_ptr(),
                  self.ep_step.data_ptr(), self.obs.data_ptr(), self.obs32.data_ptr(), self.reset_count.data_ptr(),
                  self.reset_noise.data_ptr(), stream_ptr())

    def _host_reset(self, mask=None):
        """The fixed start, P/envs/pvtol_env.py:230-251.  Of its 7 components a start offset (dx, dy) (the device
        reset with an ``init_spread``; ``envs.PvtolEnv.reset(offset=)`` on the host) moves three: x (0) and y (1), and
        the safety operator's x (6), which the reference sets to the vehicle's x at every reset and therefore moves
        by dx.  The tilt (2), the velocities (3, 4) and the thrust (5) stay 0, 0, 0, 1.  The reference's
        ``last_goal_dist`` is re-derived from the position too, but no output of the step reads it and the device
        simulator does not keep it.  The observation follows from the state by ``step``'s formulas."""
        m = self._all if mask is None else torch.as_tensor(mask, device=self.device).bool()
        self.state[m] = torch.tensor(self.start_state, dtype=torch.float64, device=self.device)
        self.ep_step[m] = 0
        st = self.state
        rx, ry = self.goal_pos[0] - st[:, 0], self.goal_pos[1] - st[:, 1]
        c, s = torch.cos(st[:, 2]), torch.sin(st[:, 2])
        v0, v1 = rx * c + ry * s, -rx * s + ry * c
        n = torch.sqrt(v0 * v0 + v1 * v1) + 0.001
        self.obs.copy_(torch.stack([st[:, 0], st[:, 1], c, s, st[:, 3], st[:, 4], st[:, 5], st[:, 6], v0 / n, v1 / n,
                                    torch.exp(-torch.sqrt(rx * rx + ry * ry))], 1))
        return self.obs

    def step(self, action):
        a = self._action(action)
        par = _dparams(self.dt, self.goal_pos[0], self.goal_pos[1], self.goal_size, self.reward_goal, self.hazards_radius,
                       self.safety_operator_follow, self.little_b, self.capital_b)
        _lib.call("nlbac_pvtol_env_step", self.n, par, int(self.max_episode_steps), self._hz.data_ptr(),
                  self._hz.shape[0], a.data_ptr(), self.state.data_ptr(), self.ep_step.data_ptr(), self.obs.data_ptr(),
                  self.reward.data_ptr(), self.constraint.data_ptr(), self.signal.data_ptr(), self.lya_pre.data_ptr(),
                  self.done.data_ptr(), self.info.data_ptr(), stream_ptr())
        out = (self.obs, self.reward, self.constraint) + ((self.signal,) if self.barrier else ())
        return out + (self.lya_pre, self.obs, self.done, self._info("goal_met"))


class DeviceSimulatedCarsEnv(SimulatedCarsSpec, _DeviceEnv):
    """C/envs/simulated_cars_env.py:66-146 for ``n_envs`` environments; the initial velocity noise of ``reset`` is drawn
    on the host from numpy's global generator, one draw per environment reset (as the reference does per reset).

    ``device_resets=True``: the reset is one launch (``nlbac_cars_env_reset``) and lane i's k-th offset is a
    counter-based draw at (seed, i, k) made on the device — it depends on neither the lane count nor on when the reset
    happened, and numpy's global generator is neither seeded nor read.  ``reset_noise`` holds every lane's last offset,
    ``reset_count`` the number of its resets (the constructor's included)."""
    state_dim, obs_dim, lya_dim, act_dim = 10, 10, 4, 1
    should_keep_thre, reward_goal = 0.5, 2.0

    def __init__(self, n_envs, seed=0, device="cuda", device_resets=False):
        SimulatedCarsSpec.__init__(self, seed)
        self.device_resets = bool(device_resets)
        if not self.device_resets:
            np.random.seed(seed)
        self._common(n_envs, device)
        self.t = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        if self.device_resets:
            self._device_buffers()
            self.reset_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            self.reset_noise = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.reset()

    def _noise(self, noise):
        if noise is None:
            return None
        return torch.as_tensor(noise, dtype=torch.float64, device=self.device).reshape(self.n).contiguous()

    def _launch_reset(self, flags, noise=None):
        nz = self._noise(noise)
        _lib.call("nlbac_cars_env_reset", self.n, None if flags is None else flags.data_ptr(), self.reset_seed,
                  None if nz is None else nz.data_ptr(), self.state.data_ptr(), self.t.data_ptr(),
                  self.ep_step.data_ptr(), self.obs.data_ptr(), self.obs32.data_ptr(), self.reset_count.data_ptr(),
                  self.reset_noise.data_ptr(), stream_ptr())

    def reset(self, mask=None, noise=None):
        """``noise``: the N(0, 0.5) initial-velocity offsets to use, one per environment (default, host mode: one draw
        from numpy's global generator per environment that is reset, in index order; device mode: the lane's
        counter-based draw)."""
        if not self.device_resets:
            return self._host_reset(mask, noise)
        self._launch_reset(None if mask is None else self._flags(torch.as_tensor(mask, device=self.device).bool()), noise)
        return self.obs

    def reset_done(self, done=None, noise=None):
        """``_DeviceEnv.reset_done``; ``noise``: as for ``reset`` — a float64 (n,) device tensor, or a sequence that is
        uploaded.  Device mode returns the persistent ``self.obs32``, which the next call overwrites."""
        done = self.done if done is None else done
        if not self.device_resets:
            d = torch.as_tensor(done, device=self.device)
            self.reset(d if d.dtype == torch.bool else d > 0, noise)
            return self.obs.to(torch.float32).clone()
        self._launch_reset(self._flags(done), noise)
        return self.obs32

    def _host_reset(self, mask=None, noise=None):
        m = (np.ones(self.n, dtype=bool) if mask is None else torch.as_tensor(mask).bool().cpu().numpy())
        for i in np.nonzero(m)[0]:
            st = np.zeros(10)
            st[::2] = [42.0, 34.0, 26.0, 18.0, 10.0]
            st[1::2] = 3.0 + (np.random.normal(0, 0.5) if noise is None else float(noise[i]))
            st[7] = 3.0
            self.state[i] = torch.from_numpy(st).to(self.device)
        mt = torch.from_numpy(m).to(self.device)
        self.t[mt] = 0.0
        self.ep_step[mt] = 0
        o = self.state.clone()
        o[:, ::2] /= 100.0
        o[:, 1::2] /= 30.0
        self.obs.copy_(o)
        return self.obs

    def step(self, action):
        a = self._action(action)
        par = _dparams(self.dt, self.kp, self.k_brake, self.should_keep, self.should_keep_thre, self.reward_goal)
        _lib.call("nlbac_cars_env_step", self.n, par, int(self.max_episode_steps), a.data_ptr(), self.state.data_ptr(),
                  self.t.data_ptr(), self.ep_step.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                  self.constraint.data_ptr(), self.lya_pre.data_ptr(), self.lya_next.data_ptr(), self.done.data_ptr(),
                  self.info.data_ptr(), stream_ptr())
        return (self.obs, self.reward, self.constraint, self.lya_pre, self.lya_next, self.done, self._info("reached"))


class DeviceQuadrotorLikeEnv(_StartSpread, QuadrotorLikeSpec, _DeviceEnv):
    """``envs.QuadrotorLikeEnv`` for ``n_envs`` environments (``QuadrotorLikeSpec``'s docstring has the step; no
    reference code exists for this task).  ``step`` always returns the barrier copies' 8-tuple; the Lyapunov inputs are
    the observations before / after the step.

    ``init_spread=(sx, sz)``: every reset draws its start position, x = 1.5 + sx (2 u0 - 1), z = 0.3 + sz (2 u1 - 1),
    so that N lanes are N different episodes.  The draws are made on the device by the reset's own launch
    (``nlbac_quadrotor_env_reset``) from counters (seed, lane, reset number), as SimulatedCars' are, and need
    ``device_resets=True`` (``_StartSpread``).  ``reset_noise`` (n, 2) holds every lane's last (dx, dz), ``reset_count``
    the number of its resets (the constructor's included).  Without a spread the start is the fixed row and device mode
    is the generic ``nlbac_env_reset_rows``."""
    state_dim, obs_dim, lya_dim, act_dim = 6, 6, 6, 2
    barrier = True                             # (the task has a learned barrier and no other form)

    def __init__(self, n_envs, seed=0, device="cuda", device_resets=False, init_spread=(0.0, 0.0)):
        spread = _spread_of(type(self), init_spread, device_resets)
        QuadrotorLikeSpec.__init__(self, seed)
        self.init_spread, self.device_resets = spread, bool(device_resets)
        self._common(n_envs, device)
        self._par = _dparams(self.dt, self.MASS, self.IYY, self.ARM, self.G, self.goal_pos[0], self.goal_pos[1],
                             self.goal_size, self.reward_goal, self.x_range[0], self.x_range[1], self.z_range[0],
                             self.z_range[1], self.obstacle[0], self.obstacle[1], self.obstacle_radius, self.D1, self.D2,
                             self.crash_x[0], self.crash_x[1], self.crash_z[0], self.crash_z[1], self.crash_theta)
        if self.device_resets:
            self._device_buffers()
            self._capture_start()
            self._spread_buffers(seed)
            self._reset_par = _dparams(*(tuple(self.start_state) + spread))
        self.reset()

    def _host_reset(self, mask=None):
        m = self._all if mask is None else torch.as_tensor(mask, device=self.device).bool()
        self.state[m] = torch.tensor(self.start_state, dtype=torch.float64, device=self.device)
        self.ep_step[m] = 0
        self.obs.copy_(self.state)
        return self.obs

    def _launch_spread_reset(self, flags, noise):
        _lib.call("nlbac_quadrotor_env_reset", self.n, flags, self.reset_seed, self._reset_par, noise,
                  self.state.data_ptr(), self.ep_step.data_ptr(), self.obs.data_ptr(), self.obs32.data_ptr(),
                  self.reset_count.data_ptr(), self.reset_noise.data_ptr(), stream_ptr())

    def step(self, action):
        a = self._action(action)
        _lib.call("nlbac_quadrotor_env_step", self.n, self._par, int(self.max_episode_steps), a.data_ptr(),
                  self.state.data_ptr(), self.ep_step.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                  self.constraint.data_ptr(), self.signal.data_ptr(), self.lya_pre.data_ptr(), self.done.data_ptr(),
                  self.info.data_ptr(), stream_ptr())
        return (self.obs, self.reward, self.constraint, self.signal, self.lya_pre, self.obs, self.done,
                self._info("goal_met"))


def make(name, n_envs, seed=0, device="cuda", device_resets=False, **kw):
    """``Unicycle`` / ``UnicycleBarrier`` / ``SimulatedCars`` / ``Pvtol`` / ``PvtolBarrier`` / ``QuadrotorLike``, batched
    on the device; ``device_resets=True``: resets on the device (one launch per ``reset_done``).  ``**kw`` goes to the
    class: ``init_spread=(sx, sy)`` for every task but SimulatedCars, whose draw is its own."""
    if name == "QuadrotorLike":
        return DeviceQuadrotorLikeEnv(n_envs, seed, device=device, device_resets=device_resets, **kw)
    if name in ("Unicycle", "UnicycleBarrier"):
        return DeviceUnicycleEnv(n_envs, seed, barrier=name.endswith("Barrier"), device=device,
                                 device_resets=device_resets, **kw)
    if name == "SimulatedCars":
        return DeviceSimulatedCarsEnv(n_envs, seed, device=device, device_resets=device_resets, **kw)
    if name in ("Pvtol", "PvtolBarrier"):
        return DevicePvtolEnv(n_envs, seed, barrier=name.endswith("Barrier"), device=device,
                              device_resets=device_resets, **kw)
    raise Exception("Dynamics mode not supported.")
