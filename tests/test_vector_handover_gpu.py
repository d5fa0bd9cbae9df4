"""GPU: the vectorised driver's backup-controller hand-over on the device (``nlbac_amd.vector_handover``,
``train.train_vectorized(handover=...)``).  Lane i must be ``train.train``'s loop for one environment as far as
controllers and replays go: the per-lane state machines against the host classes on the reference's own traces, the
compaction of the kept rows and the head in device memory against host-built lists, the device-head draw against
``nlbac_sample_rows``, a run whose hand-over never fires against the plain run bit for bit, and a run that hands over
and comes back against the host simulator with the host class."""
import os
import types

import numpy as np
import pytest
import torch

from nlbac_amd import _lib, envs, train, vector_handover
from nlbac_amd.arena import stream_ptr
from nlbac_amd.envs import device as denv
from nlbac_amd.sac_cbf_clf.replay_memory import DeviceKeptReplay, DeviceReplayMemory
from nlbac_amd.sac_cbf_clf.update_plan import _Layout
from nlbac_amd.train import train_vectorized

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Host-side margins: the nearest a compared quantity that is not a single IEEE operation of the inputs comes to its
# threshold, per trace — figures of the traces themselves (properties of the fixtures and of the host classes, not of
# the code under test), asserted so that a rounding difference on the device could not hide behind a flag that happens
# not to flip: 7.5e-4 for Unicycle's ``moved`` against 0.01, 3.4e-4 for Pvtol's against 0.015, 0.5 for the cars' gaps
# against 2.5 (0.5 less a few ulps of the gaps: 2.0 and 3.0 come out of obs * 100 a rounding off).  The device's inputs
# are the host's own bits there.  In the driver test (5) they are a simulator's that agrees with the host's to 1e-12,
# and the script's margin is 4.0e-4.  That the device rounds every operation as numpy does is test 6's business.
MARGINS = {"Unicycle": 7.5e-4, "Pvtol": 3.4e-4, "SimulatedCars": 0.5 - 1e-12}
DRIVER_MARGIN = 4.0e-4


def layout(obs_dim, act_dim, lya_dim):
    return _Layout(types.SimpleNamespace(obs_dim=obs_dim, act_dim=act_dim, lya_dim=lya_dim, has_signal=False))


def host_flags(kind, env, k, lya, next_lya, obs, reached, done, first_backup_episode=None):
    """``use_backup`` before every step of one lane as ``train.train`` evaluates it, and the least distance of a
    compared float64 quantity that is not a single IEEE operation of the inputs (``moved``, the distance from the
    hand-over point while it is compared, the cars' gaps) from its threshold."""
    ho = train.make_handover(kind, env, True)
    if first_backup_episode is not None:
        ho.first_backup_episode = first_backup_episode
    e, margin = 0, np.inf
    ho.begin_episode(e)
    flags = np.zeros(len(k), dtype=bool)
    for t in range(len(k)):
        flags[t] = ho.use_backup
        if flags[t]:
            ho.on_backup_action()
        was = bool(getattr(ho, "backup", False) or getattr(ho, "obs_b", False))
        ho.after_step(int(k[t]), lya[t], next_lya[t], obs[t], {"reached": reached[t]})
        if kind == "SimulatedCars":
            d34, d45 = obs[t][4] * 100.0 - obs[t][6] * 100.0, obs[t][6] * 100.0 - obs[t][8] * 100.0
            margin = min(margin, abs(d34 - ho.GAP), abs(d45 - ho.GAP))
        elif k[t] >= ho.MIN_CHECK_STEP:
            d = ho.positions[-1] - ho.positions[-ho.LOOKBACK]
            margin = min(margin, abs(d[0] * d[0] + d[1] * d[1] - ho.STUCK2))
            now = bool(getattr(ho, "backup", False) or getattr(ho, "obs_b", False))
            if was or now:
                dx, dy = next_lya[t][0] - ho.x0, next_lya[t][1] - ho.y0
                margin = min(margin, abs(dx * dx + dy * dy - ho.AWAY2))
        if done[t]:
            e += 1
            ho.begin_episode(e)
    return flags, margin


# ---------------------------------------------------------------------------------------------------------------------
# 1. the state machines against the host classes on the reference's own traces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,kind,n_flagged", [("Unicycle", "Unicycle", 42), ("Pvtol", "Pvtol", 180),
                                                    ("SimulatedCarsHandover", "SimulatedCars", 234)])
def test_lanes_follow_the_host_classes_on_the_reference_traces(fixture, kind, n_flagged):
    g = np.load(os.path.join(GOLD, "driver_%s.npz" % fixture))
    done = g["done"].astype(bool)
    T = len(done)
    ends = np.flatnonzero(done)
    assert ends[-1] == T - 1
    starts = np.concatenate([[0], ends[:-1] + 1])
    E = len(ends)
    k = np.concatenate([np.arange(1, e - s + 2) for s, e in zip(starts, ends)])        # step within the episode
    env = envs.make("Pvtol", 0) if kind == "Pvtol" else None
    # precondition: the host class on the unrotated trace reproduces the reference's own decisions
    f0, m0 = host_flags(kind, env, k, g["lya"], g["next_lya"], g["obs"], g["reached"], done)
    assert np.array_equal(f0.astype(np.int64), g["backup"]) and g["backup"].sum() == n_flagged > 0
    N = 70                                                                             # two waves, the second ragged
    order = []
    for r in range(E):                                                                 # episodes rotated by r
        eps = [np.arange(starts[e % E], ends[e % E] + 1) for e in range(r, r + E)]
        order.append(np.concatenate(eps))
    expect, margin = [], m0
    for r in range(E):
        o = order[r]
        f, m = host_flags(kind, env, k[o], g["lya"][o], g["next_lya"][o], g["obs"][o], g["reached"][o], done[o])
        expect.append(f)
        margin = min(margin, m)
    assert margin >= MARGINS[kind], "a compared quantity comes within %.3e of its threshold" % margin
    lane_order = np.stack([order[j % E] for j in range(N)], axis=1)                    # (T, N) trace step of lane j at step t
    dev = torch.device("cuda")
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a[lane_order]), dtype=dt, device=dev)
    lya, nlya, obs = up(g["lya"], torch.float64), up(g["next_lya"], torch.float64), up(g["obs"], torch.float64)
    reached, dn, kk = up(g["reached"], torch.float64), up(done, torch.int32), up(k, torch.int32)
    lay = layout(obs.shape[2], 1, lya.shape[2])
    params = vector_handover.params_for(kind, env)
    ho = vector_handover.VectorHandover(kind, N, dev, params)
    got = torch.zeros(T, N, dtype=torch.bool, device=dev)
    for t in range(T):
        got[t] = ho.flags
        ho.step(lay, lya[t], nlya[t], obs[t], reached[t], dn[t], kk[t])
    got = got.cpu().numpy()
    want = np.stack([expect[j % E] for j in range(N)], axis=1)
    assert np.array_equal(got[:, 0].astype(np.int64), g["backup"]), "lane 0 is not the reference's trace"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "first differing (step, lane): %s" % bad[:5].tolist()
    assert ho.backup_steps() == int(want.sum())


# ---------------------------------------------------------------------------------------------------------------------
# 2. compaction, head and stamps
# ---------------------------------------------------------------------------------------------------------------------
def assemble(lay, obs, action, reward, constraint, lya, nlya, nobs, done, ep_step, dt, max_steps):
    """The rows of a vector step as ``train_vectorized`` assembles them without hand-over."""
    rows = torch.zeros(obs.shape[0], lay.LD, dtype=torch.float32, device=obs.device)
    t = ep_step.to(torch.float32)
    timeout = ep_step >= max_steps
    rows[:, lay.obs:lay.obs + lay.obs_dim] = obs
    rows[:, lay.act:lay.act + lay.act_dim] = action
    rows[:, lay.rew], rows[:, lay.con] = reward.float(), constraint.float()
    rows[:, lay.lya:lay.lya + lay.lya_dim] = lya.float()
    rows[:, lay.nlya:lay.nlya + lay.lya_dim] = nlya.float()
    rows[:, lay.nobs:lay.nobs + lay.obs_dim] = nobs.float()
    rows[:, lay.mask] = torch.where(timeout, torch.ones_like(reward), 1.0 - done.to(reward.dtype)).float()
    rows[:, lay.t], rows[:, lay.nt] = t * float(dt), (t + 1.0) * float(dt)
    return rows


@pytest.mark.parametrize("shift", [0, -1])
def test_kept_rows_are_compacted_in_lane_order_behind_a_device_head(shift):
    N, cap, pushes, dt, max_steps = 300, 1000, 12, 0.02, 30                    # two workgroups, the second partial
    dev = torch.device("cuda")
    lay = layout(7, 2, 2)
    agent = types.SimpleNamespace(lay=lay, device=dev)
    node = DeviceReplayMemory(cap, 0, agent, device_rng=True)
    kept = DeviceKeptReplay(cap, 0, agent, draws_from=node)
    ho = vector_handover.VectorHandover("Unicycle", N, dev, vector_handover.params_for("Unicycle", memory_t_shift=shift))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    rnd = lambda *s, dtype=torch.float64: torch.randn(*s, generator=gen, device=dev, dtype=dtype)
    node_want = torch.zeros(cap, lay.LD, device=dev)
    kept_want = torch.zeros(cap, lay.LD, device=dev)
    node_pos = kept_total = 0
    for p in range(pushes):
        flags = torch.rand(N, generator=gen, device=dev) < 0.5
        if p == 3:
            flags[:] = False                                                   # all kept
        if p == 7:
            flags[:] = True                                                    # none kept
        ho.flags.copy_(flags)                                                  # (prescribed)
        ep_step = torch.randint(1, 41, (N,), generator=gen, device=dev, dtype=torch.int32)   # (< 50: no check changes a flag)
        done = (torch.rand(N, generator=gen, device=dev) < 0.3).to(torch.int32)
        obs, action = rnd(N, 7, dtype=torch.float32), rnd(N, 2, dtype=torch.float32)
        reward, constraint, lya, nlya, nobs = rnd(N), rnd(N), rnd(N, 2), rnd(N, 2), rnd(N, 7)
        info0 = torch.zeros(N, 3, dtype=torch.float64, device=dev)[:, 0]
        ho.push(node, kept, obs, action, reward, constraint, lya, nlya, nobs, info0, done, ep_step, dt, max_steps)
        rows = assemble(lay, obs, action, reward, constraint, lya, nlya, nobs, done, ep_step, dt, max_steps)
        idx = (node_pos + torch.arange(N, device=dev)) % cap
        node_want[idx] = rows
        node_pos = (node_pos + N) % cap
        krows = rows[~flags].clone()
        if shift:
            ts = (ep_step[~flags] + shift).to(torch.float32)
            krows[:, lay.t], krows[:, lay.nt] = ts * float(dt), (ts + 1.0) * float(dt)
            if len(krows):                                                     # (the stamps moved by dt, the NODE's did not)
                np.testing.assert_allclose((rows[~flags][:, lay.t] - krows[:, lay.t]).cpu().numpy(), -shift * dt, atol=1e-6)
        kidx = (kept_total + torch.arange(len(krows), device=dev)) % cap
        kept_want[kidx] = krows
        kept_total += len(krows)
        assert torch.equal(node.rows, node_want), "push %d: the NODE ring does not hold every row" % p
        assert torch.equal(kept.rows, kept_want), "push %d: the controller ring is not the kept rows in lane order" % p
        head = kept.head.cpu().tolist()
        assert head[kept.half] == [kept_total % cap, min(cap, kept_total)], (p, head, kept.half)
        assert not bool(ho.flags.any())                                        # (the state machine: nothing handed over)
        assert (node.position, len(node)) == (node_pos, min(cap, (p + 1) * N))
    assert kept_total > cap and kept.refresh_len() == cap == len(kept)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the draw
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [10, 700])
def test_device_head_draw_is_the_by_value_draw(length):
    dev = torch.device("cuda")
    cap, ld, batch, n_eps, seed, draw = 1000, 28, 64, 130, 0x1234567890ABCDEF, 7
    ring = torch.randn(cap, ld, device=dev)
    head = torch.tensor([[3, 999], [5, length]], dtype=torch.int64, device=dev)      # (half 1 is the one named)
    a, b = torch.zeros(batch, ld, device=dev), torch.zeros(batch, ld, device=dev)
    ea, eb = torch.zeros(n_eps + 2, device=dev), torch.zeros(n_eps + 2, device=dev)
    _lib.call("nlbac_sample_rows", ring.data_ptr(), length, ld, batch, a.data_ptr(), ea.data_ptr(), n_eps, seed, draw,
              stream_ptr())
    _lib.call("nlbac_sample_rows_head", ring.data_ptr(), head.data_ptr(), 1, cap, ld, batch, b.data_ptr(), eb.data_ptr(),
              n_eps, seed, draw, stream_ptr())
    assert torch.equal(a, b) and torch.equal(ea, eb)
    assert bool((ea[:n_eps] != 0).all()) and bool((ea[n_eps:] == 0).all())
    assert bool((a.abs().sum(1) > 0).all())
    # a length of 0 copies nothing
    head[1, 1] = 0
    b.fill_(-7.0)
    _lib.call("nlbac_sample_rows_head", ring.data_ptr(), head.data_ptr(), 1, cap, ld, batch, b.data_ptr(), None, 0, seed,
              draw, stream_ptr())
    assert bool((b == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. an inert hand-over is the plain run
# ---------------------------------------------------------------------------------------------------------------------
def run(env_name, n_envs, iters, handover, seed=0):
    from test_agent_parity_gpu import make_agent
    agent, spec = make_agent(64, 64, seed, "euler", env_name, {"Unicycle": 50.0, "Pvtol": 0.8}[env_name])
    env = denv.make(env_name, n_envs, seed=seed)
    env.max_episode_steps = 25
    args = types.SimpleNamespace(replay_size=4096, seed=seed, start_steps=4 * n_envs, batch_size=64, updates_per_step=1,
                                 NODE_model_update_interval=10)
    memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    ctrl = []
    upd = agent.update_parameters
    agent.update_parameters = lambda *a: (ctrl.append(a[0]), upd(*a))[1]
    if handover:
        handover = vector_handover.params_for(env_name, env, first_backup_episode=2 ** 30)
    res = train_vectorized(agent, env, args, iters * n_envs, log=lambda *a: None, memory=memory, handover=handover)
    torch.cuda.synchronize()
    return agent, memory, res, ctrl[-1]


@pytest.mark.parametrize("env_name", ["Unicycle", "Pvtol"])
def test_a_handover_that_never_fires_is_the_plain_run(env_name):
    N, iters = 16, 60
    a0, m0, r0, c0 = run(env_name, N, iters, None)
    a1, m1, r1, c1 = run(env_name, N, iters, True)
    assert c0 is m0 and isinstance(c1, DeviceKeptReplay) and c1 is not m1
    assert r1.pop("backup_steps") == 0 and "backup_steps" not in r0
    assert r0 == r1 and r0["updates"] == iters - (64 // N)
    for x, y in zip(a0.arenas, a1.arenas):
        assert torch.equal(x.theta, y.theta), "the inert hand-over run differs from the plain run"
    assert torch.equal(m0.rows, m1.rows) and (m0.position, len(m0), m0._draws) == (m1.position, len(m1), m1._draws)
    assert torch.equal(c1.rows, m1.rows) and c1.refresh_len() == len(m1)      # every row was kept


# ---------------------------------------------------------------------------------------------------------------------
# 5. the driver hands over and comes back
# ---------------------------------------------------------------------------------------------------------------------
def host_driver_flags(iters, max_steps, forward, backup_action):
    """{lane parity: flags per step} from the host simulator with the host class under the stubs' script (even lanes
    stand still, odd lanes drive forward, the backup controller drives fast), and the margin of ``host_flags``."""
    want, margin = {}, np.inf
    for parity in (0, 1):
        env = envs.make("Unicycle", 0)
        env.max_episode_steps = max_steps
        ho = train._UnicycleHandover(env)
        ho.first_backup_episode = 0
        e = 0
        ho.begin_episode(e)
        env.reset()
        flags = np.zeros(iters, dtype=bool)
        for t in range(iters):
            flags[t] = ho.use_backup
            if flags[t]:
                ho.on_backup_action()
                action = backup_action
            else:
                action = np.array([forward if parity else 0.0, 0.0], dtype=np.float32)
            was = ho.backup
            out = env.step(action.astype(np.float64))
            lya_in, next_lya_in, done, info = out[-4:]
            k = (t % max_steps) + 1
            ho.after_step(k, lya_in, next_lya_in, out[0], info)
            if k >= ho.MIN_CHECK_STEP:
                d = ho.positions[-1] - ho.positions[-ho.LOOKBACK]
                margin = min(margin, abs(d[0] * d[0] + d[1] * d[1] - ho.STUCK2))
                if was or ho.backup:
                    dx, dy = next_lya_in[0] - ho.x0, next_lya_in[1] - ho.y0
                    margin = min(margin, abs(dx * dx + dy * dy - ho.AWAY2))
            assert bool(done) == (k == max_steps), "the script ends an episode early: pick another"
            if done:
                e += 1
                ho.begin_episode(e)
                env.reset()
        want[parity] = flags
    return want, margin


def test_the_driver_hands_over_and_comes_back(monkeypatch):
    from test_agent_parity_gpu import make_agent
    N, iters, max_steps, batch = 16, 100, 80, 64
    forward, backup_action = np.float32(1.0), np.array([3.0, 0.0], dtype=np.float32)
    # ---- expected: the host simulator with the host class, one run per kind of lane
    want, margin = host_driver_flags(iters, max_steps, forward, backup_action)
    assert margin >= DRIVER_MARGIN, margin
    on = np.flatnonzero(np.diff(want[0].astype(int)) == 1)
    off = np.flatnonzero(np.diff(want[0].astype(int)) == -1)
    assert len(on) >= 1 and len(off) >= 1 and off[0] > on[0] and off[0] % max_steps != max_steps - 1, \
        "even lanes must hand over and come back within an episode"
    assert not want[1].any(), "odd lanes must never hand over"
    want = np.stack([want[j % 2] for j in range(N)], axis=1)                   # (iters, N)
    # ---- the vectorised driver with stub policies
    agent, spec = make_agent(batch, 64, 0, "euler", "Unicycle", 50.0)
    dev = agent.device
    primary = torch.zeros(N, 2, device=dev)
    primary[1::2, 0] = float(forward)
    backup = torch.as_tensor(backup_action, device=dev).repeat(N, 1)
    agent.policy.sample = lambda obs, eps=None: (primary.clone(), None, None)
    agent.backup_policy.sample = lambda obs, eps=None: (backup.clone(), None, None)
    env = denv.make("Unicycle", N, seed=0)
    env.max_episode_steps = max_steps
    args = types.SimpleNamespace(replay_size=4096, seed=0, start_steps=0, batch_size=batch, updates_per_step=1,
                                 NODE_model_update_interval=10)
    memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    calls, per_step, seen, ctrl, refreshes = [], [], [], [], []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    real_refresh = DeviceKeptReplay.refresh_len
    monkeypatch.setattr(DeviceKeptReplay, "refresh_len", lambda self: (refreshes.append(len(seen)), real_refresh(self))[1])
    upd = agent.update_parameters
    agent.update_parameters = lambda *a: (ctrl.append(a[0]), upd(*a))[1]

    def check(it, rows, flags):
        per_step.append(list(calls))
        del calls[:]
        seen.append((rows.clone(), flags.clone()))
    res = train_vectorized(agent, env, args, iters * N, log=lambda *a: None, memory=memory, check=check,
                           handover=vector_handover.params_for("Unicycle", env, first_backup_episode=0))
    torch.cuda.synchronize()
    monkeypatch.undo()
    lay, kept = agent.lay, ctrl[-1]
    got = torch.stack([f for _, f in seen]).cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "first differing (step, lane): %s" % bad[:5].tolist()
    n_flagged = int(want.sum())
    assert res["backup_steps"] == n_flagged > 0 and res["steps"] == iters * N
    # flagged steps carry the backup stub's action in the NODE ring, the others the primary's
    acts = torch.stack([r[:, lay.act:lay.act + 2] for r, _ in seen])
    w = torch.as_tensor(want, device=dev)
    assert torch.equal(acts, torch.where(w[:, :, None], backup[None], primary[None]))
    assert torch.equal(memory.rows[:iters * N], torch.cat([r for r, _ in seen]))
    # the controller replay: everything but the flagged steps, none of them among its rows
    assert len(memory) == iters * N and kept.refresh_len() == len(memory) - n_flagged
    key = lambda r: torch.cat([r[:, lay.obs:lay.obs + lay.obs_dim], r[:, lay.t:lay.t + 1]], 1)
    all_rows = torch.cat([r for r, _ in seen])
    flat = w.reshape(-1)
    assert torch.equal(kept.rows[:len(memory) - n_flagged], all_rows[~flat]), "the controller replay is not the kept rows in order"
    hit = (key(all_rows[flat])[:, None, :] == key(kept.rows[:len(kept)])[None, :, :]).all(2)
    assert not bool(hit.any()), "a flagged step's stamp and observation are in the controller replay"
    # launches: per_step[j] holds the calls between check j-1 and check j, i.e. the updates of step j-1 (once the gate
    # has passed), the simulator and the hand-over's two launches of step j
    kept_before = np.cumsum((~want).sum(1))
    gate = int(np.argmax(kept_before > batch))                                 # the step whose push opens the gate
    assert res["updates"] == iters - gate
    step = per_step[gate + 3]
    assert step.count("nlbac_vector_step_rows") == 1 and step.count("nlbac_ring_append_kept") == 1
    assert step.count("nlbac_unicycle_env_step") == 1 and step.count("nlbac_sample_rows_head") == 1
    assert refreshes == list(range(1, gate + 2)), "refresh_len is read once per step until the gate has passed, then never"


# ---------------------------------------------------------------------------------------------------------------------
# 6. no contraction: inputs on which a fused multiply-add decides otherwise than numpy
# ---------------------------------------------------------------------------------------------------------------------
def _contraction_cases():
    """(dx, dy, two-rounding sum, fused sum) with fused != two-rounding, for both operands a backend may fuse and both
    directions of the difference.  The fused value is formed exactly (fractions; float() of a Fraction rounds once)."""
    from fractions import Fraction as F
    rng, found = np.random.default_rng(0), {}
    while len(found) < 4:
        dx, dy = (float(v) for v in rng.uniform(0.05, 0.1, 2))
        plain = dx * dx + dy * dy
        for which, fused in (("x", float(F(dx) * F(dx) + F(dy * dy))), ("y", float(F(dx * dx) + F(dy) * F(dy)))):
            if fused != plain:
                found.setdefault((which, fused > plain), (dx, dy, plain, fused))
    return list(found.values())


def test_moved_is_rounded_as_numpy_rounds_it_not_fused():
    """``moved = dx*dx + dy*dy`` with a threshold BETWEEN numpy's value and the value a fused multiply-add gives: the
    flag must be the host class's.  One lane state per case, 64 lanes each, one check (step 50) that hands over or not."""
    dev = torch.device("cuda")
    N, lay = 64, layout(7, 2, 2)
    for dx, dy, plain, fused in _contraction_cases():
        stuck2 = min(plain, fused)
        ho_host = train._UnicycleHandover(None)
        ho_host.first_backup_episode, ho_host.CHECKS, ho_host.STUCK2 = 0, 1, stuck2
        ho_host.begin_episode(0)
        params = vector_handover.params_for("Unicycle", first_backup_episode=0, checks=1, stuck2=stuck2)
        ho = vector_handover.VectorHandover("Unicycle", N, dev, params)
        z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev)
        for k in range(1, 51):
            pos = np.array([dx, dy]) if k == 50 else np.zeros(2)          # (the position 39 steps before step 50 is 0)
            ho_host.after_step(k, np.zeros(2), pos, None, {})
            nl = torch.as_tensor(pos, device=dev).repeat(N, 1)
            ho.step(lay, z(N, 2), nl, z(N, 7), z(N), z(N, dtype=torch.int32), torch.full((N,), k, dtype=torch.int32, device=dev))
        assert ho_host.use_backup == (plain <= stuck2)
        assert ho.flags.cpu().tolist() == [ho_host.use_backup] * N, \
            "moved for (%r, %r): numpy %r, fused %r, threshold %r" % (dx, dy, plain, fused, stuck2)


def test_cars_gap_is_rounded_as_numpy_rounds_it_not_fused():
    """The same for ``d45 = obs[6]*100 - obs[8]*100`` against the gap (a backend may fuse either product)."""
    from fractions import Fraction as F
    dev = torch.device("cuda")
    N, lay = 64, layout(10, 1, 4)
    rng, cases = np.random.default_rng(1), {}
    while len(cases) < 2:
        o6, o8 = (float(v) for v in rng.uniform(0.1, 0.3, 2))
        plain = o6 * 100.0 - o8 * 100.0
        for fused in (float(F(o6 * 100.0) - F(o8) * 100), float(F(o6) * 100 - F(o8 * 100.0))):
            if fused != plain and plain > 0:
                cases.setdefault(fused > plain, (o6, o8, plain, fused))
    for o6, o8, plain, fused in cases.values():
        gap = max(plain, fused)                                           # d45 < gap hands over: only the smaller does
        host = train._CarsHandover(None)
        host.GAP = gap
        host.begin_episode(0)
        obs = np.zeros(10)
        obs[6], obs[8] = o6, o8
        host.after_step(1, None, None, obs, {"reached": 1.0})
        ho = vector_handover.VectorHandover("SimulatedCars", N, dev, vector_handover.params_for("SimulatedCars", gap=gap))
        z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev)
        ho.step(lay, z(N, 4), z(N, 4), torch.as_tensor(obs, device=dev).repeat(N, 1), torch.ones(N, dtype=torch.float64, device=dev),
                z(N, dtype=torch.int32), torch.ones(N, dtype=torch.int32, device=dev))
        assert host.use_backup == (plain < gap)
        assert ho.flags.cpu().tolist() == [host.use_backup] * N, (o6, o8, plain, fused, gap)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the SimulatedCars kind through the fused path: no position ring, ``reached``, the stamp shift
# ---------------------------------------------------------------------------------------------------------------------
def test_cars_trace_through_the_fused_path():
    """The scripted SimulatedCars hand-over trace through ``VectorHandover.push`` (70 lanes, episodes rotated per lane):
    the flags are the host class's, the NODE ring holds every row stamped ``k dt``, the controller ring the rows of the
    steps the primary controller took, in step and lane order, stamped ``(k - 1) dt`` (``memory_t_shift = -1``)."""
    g = np.load(os.path.join(GOLD, "driver_SimulatedCarsHandover.npz"))
    done = g["done"].astype(bool)
    ends = np.flatnonzero(done)
    starts = np.concatenate([[0], ends[:-1] + 1])
    E, T, N, dt, max_steps = len(ends), 200, 70, 0.02, int(g["meta_max_steps"])
    k = np.concatenate([np.arange(1, e - s + 2) for s, e in zip(starts, ends)])
    order = [np.concatenate([np.arange(starts[e % E], ends[e % E] + 1) for e in range(r, r + E)])[:T] for r in range(E)]
    want = np.stack([host_flags("SimulatedCars", None, k[o], g["lya"][o], g["next_lya"][o], g["obs"][o], g["reached"][o],
                                done[o])[0] for o in order], axis=1)[:, np.arange(N) % E]          # (T, N)
    assert want.any() and not want.all()
    lane_order = np.stack([order[j % E] for j in range(N)], axis=1)
    dev = torch.device("cuda")
    up = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a[lane_order]), dtype=dtype, device=dev)
    lya, nlya, nobs = up(g["lya"], torch.float64), up(g["next_lya"], torch.float64), up(g["obs"], torch.float64)
    reward, constraint = up(g["reward"], torch.float64), up(g["constraint"], torch.float64)
    reached, dn, kk = up(g["reached"], torch.float64), up(done, torch.int32), up(k, torch.int32)
    lay = layout(10, 1, 4)
    agent = types.SimpleNamespace(lay=lay, device=dev)
    cap = T * N + 100
    node = DeviceReplayMemory(cap, 0, agent, device_rng=True)
    kept = DeviceKeptReplay(cap, 0, agent, draws_from=node)
    ho = vector_handover.VectorHandover("SimulatedCars", N, dev, vector_handover.params_for("SimulatedCars"))
    assert ho.pos_ring is None and ho.params.memory_t_shift == -1
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    got, rows = torch.zeros(T, N, dtype=torch.bool, device=dev), []
    for t in range(T):
        got[t] = ho.flags
        obs = torch.randn(N, 10, generator=gen, device=dev)
        action = torch.randn(N, 1, generator=gen, device=dev)
        ho.push(node, kept, obs, action, reward[t], constraint[t], lya[t], nlya[t], nobs[t], reached[t], dn[t], kk[t], dt,
                max_steps)
        rows.append(assemble(lay, obs, action, reward[t], constraint[t], lya[t], nlya[t], nobs[t], dn[t], kk[t], dt, max_steps))
    assert np.array_equal(got.cpu().numpy(), want)
    rows = torch.cat(rows)
    assert torch.equal(node.rows[:T * N], rows)
    keep = ~torch.as_tensor(want, device=dev).reshape(-1)
    krows = rows[keep].clone()
    ts = (kk[:T].reshape(-1)[keep] - 1).to(torch.float32)
    krows[:, lay.t], krows[:, lay.nt] = ts * float(dt), (ts + 1.0) * float(dt)
    n_kept = int(keep.sum())
    assert kept.refresh_len() == n_kept == T * N - int(want.sum()) and ho.backup_steps() == int(want.sum())
    assert torch.equal(kept.rows[:n_kept], krows) and not bool(kept.rows[n_kept:].any())
