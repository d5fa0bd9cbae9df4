"""Reference-shaped training driver: the loop of ``U/main.py:20-165`` — warm-up with random
actions, one ``update_parameters`` per ``updates_per_step`` once the replay holds a batch, transitions pushed to the
controller replay and the NODE replay, and each copy's rules for handing control to the backup controller
(``U/main.py:108-142``, ``C/main.py:100-112``, ``P/main.py:128-200``; the learned-barrier copies have none) — on the
gym-free simulators of ``nlbac_amd.envs`` and the MI355X agent.  Logging is one
line per episode (the reference's wandb / spinup loggers are host tooling and out of scope).

    python -m nlbac_amd.train --env Unicycle --gamma_b 50 --max_episodes 200 --cuda --updates_per_step 2 \\
        --batch_size 128 --seed 0 --start_steps 1000          (the reference README's command line)
    python -m nlbac_amd.train --env QuadrotorLike --gamma_b 1 --cuda ...   (the Quadrotor-like task: this build's
        simulator, envs.QuadrotorLikeEnv — the reference holds no code for it)

``--device_replay`` keeps both replays in HBM (same index stream, gather on the device).
``--vector_envs N`` steps N environments on the device (``train_vectorized``); with ``--vector_handover`` each lane
also follows its copy's hand-over rules on the device (``vector_handover.py``); with ``--vector_episodes`` the
per-episode records (reward, length, safety violations, safety cost) are kept on the device (``vector_episodes.py``) and
``--vector_episode_tsv PATH`` writes them out; with ``--vector_device_resets`` finished lanes restart by one launch on
the device (SimulatedCars always does when vectorised), and with ``--vector_init_spread SX SY`` every restart draws its
start position there, so that the lanes are different episodes.  ``evaluate_vectorized`` evaluates the acting policy on
the same lanes.
``--env QuadrotorLike`` runs under both drivers like the learned-barrier copies (``has_barrier_signal``): no backup
controller, so ``--vector_handover`` raises.
"""
import argparse
import os
import time

import numpy as np


def get_args(argv=None):
    p = argparse.ArgumentParser(description="NLBAC training on MI355X (reference argument names)")
    p.add_argument('--env', default="Unicycle",
                   choices=["Unicycle", "SimulatedCars", "Pvtol", "UnicycleBarrier", "PvtolBarrier", "QuadrotorLike"])
    p.add_argument('--policy', default="Gaussian")
    p.add_argument('--gamma', type=float, default=0.99)
    p.add_argument('--tau', type=float, default=0.005)
    p.add_argument('--lr', type=float, default=0.0003)
    p.add_argument('--alpha', type=float, default=0.2)
    p.add_argument('--automatic_entropy_tuning', type=bool, default=True)
    p.add_argument('--seed', type=int, default=12345)
    p.add_argument('--batch_size', type=int, default=256)
    p.add_argument('--max_episodes', type=int, default=200)
    p.add_argument('--hidden_size', type=int, default=256)
    p.add_argument('--updates_per_step', type=int, default=1)
    p.add_argument('--start_steps', type=int, default=5000)
    p.add_argument('--target_update_interval', type=int, default=1)
    p.add_argument('--Lagrangian_multiplier_update_interval', type=int, default=8)
    p.add_argument('--NODE_model_update_interval', type=int, default=10)
    p.add_argument('--node_horizon', type=int, default=1,
                   help="H > 1: fit the NODE on trajectory windows of H consecutive transitions (multi-step rollout loss, "
                        "SAC_CBF_CLF.fit_node_windows); 1: the reference's one-step fit")
    p.add_argument('--backup_update_interval', type=int, default=20)
    p.add_argument('--replay_size', type=int, default=10000000)
    p.add_argument('--cuda', action="store_true")
    p.add_argument('--gamma_b', type=float, default=20.0)
    p.add_argument('--solver', default="euler", choices=["euler", "rk4", "dopri5"])
    p.add_argument('--output', default=None, help="directory for save_model at the reference's cadence")
    p.add_argument('--device_replay', action="store_true")
    p.add_argument('--device_rng', action="store_true",
                   help="with --device_replay: draw minibatch indices (and the policy noise) on the device instead of "
                        "replaying the reference's host random.sample stream")
    p.add_argument('--hipgraphs', action="store_true",
                   help="replay each update as hipGraphs (pays at the reference's small batch sizes, where the host's "
                        "launch rate bounds an update)")
    p.add_argument('--max_steps', type=int, default=0, help="stop after this many env steps (0: run all episodes)")
    p.add_argument('--vector_envs', type=int, default=0,
                   help="N > 0: N environments stepping on the device (train_vectorized: no transition touches the host, "
                        "primary controller only); runs --max_steps env steps (default 100000).  Every task; SimulatedCars "
                        "always resets its lanes on the device (see --vector_device_resets)")
    p.add_argument('--vector_device_resets', action="store_true",
                   help="with --vector_envs: finished lanes are restarted by one launch per vector step on the device "
                        "(envs.device.make(device_resets=True)) instead of torch ops with host syncs; SimulatedCars runs so "
                        "with or without this flag, its initial-velocity draws then come from a counter-based generator on "
                        "the device")
    p.add_argument('--vector_init_spread', nargs=2, type=float, default=None, metavar=("SX", "SY"),
                   help="with --vector_envs: every reset draws its start position on the device, uniform within SX, SY of "
                        "the task's start (envs.device.make(init_spread=(SX, SY))), so that the lanes are different "
                        "episodes; implies --vector_device_resets.  Unicycle, Pvtol, their barrier copies and QuadrotorLike "
                        "(SX, SZ); an error for SimulatedCars, whose initial-velocity draw is its own")
    p.add_argument('--vector_handover', action="store_true",
                   help="with --vector_envs: the backup controller acts where the copy's hand-over rules say so, decided "
                        "per lane on the device; its steps stay out of the controller replay")
    p.add_argument('--vector_episodes', nargs='?', type=int, const=True, default=None, metavar="CAP",
                   help="with --vector_envs: keep the per-episode records (return, length, safety violations, safety cost, "
                        "goal / time limit, backup steps) on the device, in a ring of CAP records (default max(4 N, 4096))")
    p.add_argument('--vector_episode_tsv', default=None, metavar="PATH",
                   help="with --vector_episodes: write one tab-separated line per record, under a header line, at the end of "
                        "the run")
    p.add_argument('--node_validate_every', type=int, default=0, metavar="K",
                   help="K > 0: before every update whose index is a multiple of K, measure the NODE's prediction error by "
                        "look-ahead step and state component over trajectory windows of the NODE replay "
                        "(SAC_CBF_CLF.validate_node; changes no bit of training; read and logged at the end of the run); "
                        "0: off")
    p.add_argument('--node_validate_windows', type=int, default=4096, metavar="W",
                   help="with --node_validate_every: start rows drawn per validation")
    p.add_argument('--node_validate_horizon', type=int, default=None, metavar="H",
                   help="with --node_validate_every: steps ahead (default max(node_horizon, 3))")
    p.add_argument('--node_validate_tsv', default=None, metavar="PATH",
                   help="with --node_validate_every: write one tab-separated line per (validation, step, state component), "
                        "under a header line, at the end of the run")
    return p.parse_args(argv)


class NodeValidation:
    """``--node_validate_every K`` for both drivers: ``due(updates)`` before an update, ``run`` queues one
    ``SAC_CBF_CLF.validate_node`` on the NODE replay and keeps its device tensors — no host read inside the loop —
    ``finish`` reads them all in one copy at the end of the run, turns them into ``node_fit.error_report`` dicts tagged
    with ``updates``, env ``steps``, ``horizon``, ``stride``, ``windows`` and ``solver``, logs one line per record and
    writes ``--node_validate_tsv``.  ``make`` returns None with the option off: the drivers then do nothing they did not
    do before."""
    TSV_COLUMNS = ("updates", "steps", "horizon", "stride", "windows", "windows_valid", "solver", "k", "c", "rmse", "mae",
                   "max_abs", "skill", "nrmse")

    @classmethod
    def make(cls, agent, args):
        every = int(getattr(args, "node_validate_every", 0) or 0)
        if every < 0:
            raise ValueError("--node_validate_every must be >= 0; got %d" % every)
        return cls(agent, args, every) if every > 0 else None

    def __init__(self, agent, args, every):
        self.agent, self.every = agent, every
        self.windows = int(getattr(args, "node_validate_windows", 4096))
        horizon = getattr(args, "node_validate_horizon", None)
        self.horizon = int(horizon) if horizon is not None else max(int(getattr(args, "node_horizon", 1)), 3)
        if self.windows < 1 or self.horizon < 1:
            raise ValueError("--node_validate_windows and --node_validate_horizon must be >= 1; got %d and %d"
                             % (self.windows, self.horizon))
        self.tsv = getattr(args, "node_validate_tsv", None)
        self.pending = []                    # (tags, stats, nvalid): device tensors

    def due(self, updates):
        return updates % self.every == 0

    def run(self, node_memory, updates, steps):
        agent = self.agent
        out = agent.validate_node(node_memory, self.windows, horizon=self.horizon)
        if out is not None:                  # (None: the replay does not hold one window yet)
            tags = dict(updates=updates, steps=steps, horizon=self.horizon, stride=int(agent.node_stride),
                        windows=self.windows, solver=agent.solver)
            self.pending.append((tags,) + tuple(out))

    def finish(self, log=print):
        """The records, read in one device-to-host copy."""
        if not self.pending:
            return []
        import torch
        from .node_fit import error_report
        # (one float64 row per record: the statistics, then the window count — an integer below 2^53 is exact there)
        host = torch.stack([torch.cat((st.reshape(-1), nv.reshape(1).to(torch.float64))) for _, st, nv in self.pending]).cpu()
        records = []
        for (tags, st, _), row in zip(self.pending, host):
            records.append(error_report(row[:-1].reshape(st.shape), int(row[-1]), **tags))
        self.pending = []
        for r in records:
            last = r["skill"][-1]
            worst = float(last[~last.isnan()].min()) if bool((~last.isnan()).any()) else float("nan")
            log("node validation: updates %d  steps %d  %d / %d windows  rmse by step %s  worst skill at step %d %.4f"
                % (r["updates"], r["steps"], r["windows_valid"], r["windows"],
                   " ".join("%.4g" % float(v) for v in r["rmse_step"]), r["horizon"], worst))
        if self.tsv:
            write_validation_tsv(self.tsv, records)
        return records


def write_validation_tsv(path, records):
    """One tab-separated line per (record, look-ahead step k = 1 .. H, state component c), under a header line."""
    with open(path, "w") as f:
        f.write("\t".join(NodeValidation.TSV_COLUMNS) + "\n")
        for r in records:
            H, n_s = r["rmse"].shape
            for k in range(H):
                for c in range(n_s):
                    f.write("\t".join([str(r[key]) for key in NodeValidation.TSV_COLUMNS[:7]] + [str(k + 1), str(c)] +
                                      ["%.17g" % float(r[key][k, c]) for key in NodeValidation.TSV_COLUMNS[9:]]) + "\n")


def vector_env_options(env_name, device_resets, init_spread=None):
    """The keywords ``envs.device.make`` gets from the command line: ``--vector_init_spread SX SY`` is drawn by the reset
    launch, so it implies resets on the device; SimulatedCars has a draw of its own and takes none."""
    if init_spread is None:
        return dict(device_resets=bool(device_resets))
    if env_name == "SimulatedCars":
        raise ValueError("--vector_init_spread: SimulatedCars draws its initial velocities itself and has no start spread")
    return dict(device_resets=True, init_spread=tuple(float(v) for v in init_spread))


def has_barrier_signal(env_name):
    """The tasks whose simulator returns a barrier signal and whose agent learns the barrier from it (the
    ``neural_barrier_certificate`` package): the two learned-barrier copies and the Quadrotor-like task."""
    return env_name.endswith("Barrier") or env_name == "QuadrotorLike"


class _Handover:
    """Which controller acts and which transitions reach the controller replay — the hand-over logic of the reference
    drivers, one subclass per ``main.py`` copy.  ``use_backup``: the backup controller acts this step (and the
    transition is kept out of ``memory``)."""
    first_backup_episode = None        # hand-over is allowed from this episode on (None: this copy has no backup)
    memory_t_shift = 0                 # SimulatedCars stamps the controller replay one step earlier (C/main.py:97-99)
    MIN_CHECK_STEP, LOOKBACK = 50, 40  # Unicycle / Pvtol: no check before this episode step; `moved` looks this far back

    def __init__(self, env):
        self.env = env
        self.allowed = False

    def begin_episode(self, i_episode):
        if self.first_backup_episode is not None and i_episode >= self.first_backup_episode:
            self.allowed = True

    @property
    def use_backup(self):
        return False

    def on_backup_action(self):
        pass

    def after_step(self, episode_steps, lya_in, next_lya_in, next_obs, info):
        pass


class _UnicycleHandover(_Handover):
    """U/main.py:39-142: stuck for 8 checks (the look-ahead point moved less than 0.1 in 40 steps) -> the backup
    controller for at most 30 steps or until it has moved sqrt(0.6) away; allowed after episode 3."""
    first_backup_episode = 4
    STUCK2, CHECKS, MAX_BACKUP, AWAY2 = 0.01, 8, 30, 0.6

    def begin_episode(self, i_episode):
        super().begin_episode(i_episode)
        self.backup = False
        self.positions, self.backup_time, self.violation_time = [], 0, 0
        self.x0 = self.y0 = 0.0

    @property
    def use_backup(self):
        return self.backup and self.allowed

    def on_backup_action(self):
        self.backup_time += 1

    def after_step(self, episode_steps, lya_in, next_lya_in, next_obs, info):
        self.positions.append(np.asarray(next_lya_in))
        if episode_steps < self.MIN_CHECK_STEP:
            return
        diff = self.positions[-1] - self.positions[-self.LOOKBACK]
        moved = diff[0] * diff[0] + diff[1] * diff[1]
        if self.allowed and not self.backup:
            if moved <= self.STUCK2:
                self.violation_time += 1
                if self.violation_time >= self.CHECKS:
                    self.backup, self.violation_time = True, 0
                    self.x0, self.y0 = next_lya_in[0], next_lya_in[1]
            if moved > self.STUCK2 and self.violation_time > 0:
                self.violation_time = 0
        if self.backup and self.allowed:
            if self.backup_time >= self.MAX_BACKUP:
                self.backup, self.backup_time = False, 0
            dx, dy = next_lya_in[0] - self.x0, next_lya_in[1] - self.y0
            if dx * dx + dy * dy >= self.AWAY2:
                self.backup, self.backup_time = False, 0


class _CarsHandover(_Handover):
    """C/main.py:41-112: from episode 0 on; the 4th car closer than 2.5 to the 5th while the following distance is met
    -> the backup controller, for at most 15 steps, or from 5 steps on once both gaps exceed 2.5."""
    first_backup_episode = 0
    memory_t_shift = -1
    GAP, MAX_BACKUP, MIN_BACKUP = 2.5, 15, 5

    def begin_episode(self, i_episode):
        super().begin_episode(i_episode)
        self.backup, self.backup_time = False, 0

    @property
    def use_backup(self):
        return self.backup and self.allowed

    def on_backup_action(self):
        self.backup_time += 1

    def after_step(self, episode_steps, lya_in, next_lya_in, next_obs, info):
        d34 = next_obs[4] * 100.0 - next_obs[6] * 100.0
        d45 = next_obs[6] * 100.0 - next_obs[8] * 100.0
        if self.allowed and not self.backup:
            if d45 < self.GAP and info.get('reached', 0) != 0:
                self.backup = True
        if self.backup and self.allowed:
            if self.backup_time >= self.MAX_BACKUP:
                self.backup, self.backup_time = False, 0
            if self.backup_time >= self.MIN_BACKUP and d34 > self.GAP and d45 > self.GAP:
                self.backup, self.backup_time = False, 0


class _PvtolHandover(_Handover):
    """P/main.py:40-200: two reasons to hand over, each with its own timers — trapped (moved^2 <= 0.015 in 40 steps,
    8 checks; back after 30 steps or 1.0 away) and running away from the safety operator towards the goal (back after
    15 steps or once within 0.9 operator_dist); allowed from episode 3 on."""
    first_backup_episode = 3
    STUCK2, CHECKS, MAX_BACKUP, AWAY2 = 0.015, 8, 30, 1.0          # trapped
    RUN_CHECKS, RUN_MAX_BACKUP, BACK_FRAC, X_MID = 1, 15, 0.9, 4.5   # running away from the safety operator

    def begin_episode(self, i_episode):
        super().begin_episode(i_episode)
        self.obs_b = self.y_b = False
        self.positions = []
        self.obs_time = self.y_time = self.viol_obs = self.viol_y = 0
        self.x0 = self.y0 = 0.0

    @property
    def use_backup(self):
        return (self.obs_b and self.allowed) or (self.y_b and self.allowed)

    def on_backup_action(self):
        if self.obs_b and self.y_b:
            self.obs_time += 1
            self.y_time += 1
        elif self.obs_b and not self.y_b:
            self.obs_time += 1
        else:
            self.y_time += 1

    def after_step(self, episode_steps, lya_in, next_lya_in, next_obs, info):
        self.positions.append(np.asarray(next_lya_in))
        if episode_steps < self.MIN_CHECK_STEP:
            return
        env, nx, pv = self.env, next_lya_in, lya_in
        diff = self.positions[-1] - self.positions[-self.LOOKBACK]
        moved = diff[0] * diff[0] + diff[1] * diff[1]
        if self.allowed and not self.obs_b:
            if moved <= self.STUCK2:
                self.viol_obs += 1
                if self.viol_obs >= self.CHECKS:
                    self.obs_b, self.viol_obs = True, 0
                    self.x0, self.y0 = nx[0], nx[1]
            if moved > self.STUCK2 and self.viol_obs > 0:
                self.viol_obs = 0
        if self.obs_b and self.allowed:
            if self.obs_time >= self.MAX_BACKUP:
                self.obs_b, self.obs_time = False, 0
            dx, dy = nx[0] - self.x0, nx[1] - self.y0
            if dx * dx + dy * dy >= self.AWAY2:
                self.obs_b, self.obs_time = False, 0
        running = ((nx[0] <= self.X_MID and nx[0] - pv[0] > 0 and nx[0] - nx[7] > env.operator_dist) or
                   (nx[0] > self.X_MID and nx[0] - pv[0] < 0 and nx[7] - nx[0] > env.operator_dist))
        if self.allowed and not self.y_b:
            if running:
                self.viol_y += 1
                if self.viol_y >= self.RUN_CHECKS:
                    self.y_b, self.viol_y = True, 0
            if (not running) and self.viol_y > 0:
                self.viol_y = 0
        if self.y_b and self.allowed:
            if self.y_time >= self.RUN_MAX_BACKUP:
                self.y_b, self.y_time = False, 0
            if ((nx[0] <= self.X_MID and nx[0] - nx[7] <= self.BACK_FRAC * env.operator_dist) or
                    (nx[0] > self.X_MID and nx[7] - nx[0] <= self.BACK_FRAC * env.operator_dist)):
                self.y_b, self.y_time = False, 0


def make_handover(env_name, env, has_backup):
    if not has_backup:
        return _Handover(env)          # NU / NP: one controller, every transition is kept (NU/main.py:36-90)
    return {"Unicycle": _UnicycleHandover, "SimulatedCars": _CarsHandover, "Pvtol": _PvtolHandover}[env_name](env)


def train(agent, env, dynamics_model, args, memory, node_memory, log=print, trace=None, validation=None):
    """Returns a list of per-episode dicts (reward, length, safety violations, updates).  ``trace``: a list that
    receives one (use_backup, pushed_to_memory) pair per env step (driver tests).  ``validation``: a list that receives
    the records of ``--node_validate_every`` (``NodeValidation``) at the end of the run."""
    val = NodeValidation.make(agent, args)
    barrier = has_barrier_signal(args.env)
    pvtol = args.env.startswith("Pvtol")
    has_backup = getattr(agent, "backup_policy", None) is not None
    ho = make_handover(args.env, env, has_backup and not barrier)
    total_numsteps = updates = 0
    history = []
    for i_episode in range(args.max_episodes):
        ho.begin_episode(i_episode)
        episode_reward = episode_cost = episode_steps = 0
        done = False
        obs = env.reset()
        t0 = time.perf_counter()
        while not done:
            if len(memory) > args.batch_size:
                for _ in range(args.updates_per_step):
                    extra = (i_episode,) if pvtol else ()
                    if val is not None and val.due(updates):
                        val.run(node_memory, updates, total_numsteps)
                    agent.update_parameters(memory, args.batch_size, updates, dynamics_model, node_memory,
                                            args.NODE_model_update_interval, *extra)
                    updates += 1
            warm = args.start_steps > total_numsteps
            acting_backup = ho.use_backup
            if acting_backup:
                action = agent.select_action_backup(obs, warmup=warm)
                ho.on_backup_action()
            else:
                action = agent.select_action(obs, warmup=warm)
            out = env.step(action)
            next_obs, reward, constraint = out[:3]
            sig = (out[3],) if barrier else ()
            lya_in, next_lya_in, done, info = out[-4:]
            episode_steps += 1
            total_numsteps += 1
            episode_reward += reward
            episode_cost += (info.get('num_safety_violation', 0) + info.get('num_safety_violation_obstacles', 0) +
                             info.get('num_safety_violation_safety_operator', 0) +
                             info.get('num_safety_violation_y_min', 0) + info.get('num_safety_violation_y_max', 0))
            mask = 1 if episode_steps == env.max_episode_steps else float(not done)
            row = (obs, action, reward, constraint) + sig + (lya_in, next_lya_in, next_obs, mask)
            pushed = not acting_backup
            if pushed:
                k = episode_steps + ho.memory_t_shift
                memory.push(*row, t=k * env.dt, next_t=(k + 1) * env.dt)
            node_memory.push(*row, t=episode_steps * env.dt, next_t=(episode_steps + 1) * env.dt)
            ho.after_step(episode_steps, lya_in, next_lya_in, next_obs, info)
            if trace is not None:
                trace.append((bool(acting_backup), bool(pushed)))
            obs = next_obs
            if os.environ.get("NLBAC_TRAIN_CHECKSUM") == "2" and total_numsteps % 100 == 0:
                import torch
                torch.cuda.synchronize()
                log("  step %d updates %d r %.9g a %.9g checksum %s" % (total_numsteps, updates, episode_reward, float(np.sum(action)),
                    " ".join("%.17g" % float(a.theta.double().sum()) for a in agent.arenas)))
            if args.max_steps and total_numsteps >= args.max_steps:
                done = True
        if args.output and ((i_episode % max(1, int(args.max_episodes / 2)) == 0) or i_episode == args.max_episodes - 1):
            agent.save_model(args.output)
        rec = dict(episode=i_episode, reward=float(episode_reward), length=episode_steps, violations=int(episode_cost),
                   total_steps=total_numsteps, updates=updates, seconds=time.perf_counter() - t0)
        history.append(rec)
        log("episode %(episode)d  reward %(reward).2f  length %(length)d  safety violations %(violations)d  "
            "steps %(total_steps)d  updates %(updates)d  %(seconds).1f s" % rec)
        if os.environ.get("NLBAC_TRAIN_CHECKSUM"):      # run-to-run determinism check: parameter sums to the last bit
            import torch
            torch.cuda.synchronize()
            log("  checksum " + " ".join("%.17g" % float(a.theta.double().sum()) for a in agent.arenas))
        if args.max_steps and total_numsteps >= args.max_steps:
            break
    if val is not None:
        records = val.finish(log)
        if validation is not None:
            validation.extend(records)
    return history


def _episode_base(ledger):
    """The ledger's totals when a run begins: zeros for a ledger nothing was pushed to (no host read), else one read —
    a ledger handed in from an earlier run keeps counting, and the run reports what it added."""
    if ledger.pushes == 0:
        return dict(episodes=0, violations=0, safety_cost=0.0)
    return ledger.totals()


def _episode_results(res, ledger, base, log):
    """What ``episodes=`` adds to a vectorised run's result: THIS run's records that the ring still holds (all of them
    unless the run finished more episodes than its capacity), this run's totals over its finished episodes (the
    ledger's totals now less ``base``, those at the run's beginning), the ledger itself."""
    tot = ledger.totals()
    first = max(base["episodes"], tot["episodes"] - ledger.capacity)
    if first > base["episodes"]:
        log("vectorised: the episode ledger holds the last %d of this run's %d records (capacity)"
            % (tot["episodes"] - first, tot["episodes"] - base["episodes"]))
    res["history"] = ledger.records(since=first)[1]
    res["violations"] = tot["violations"] - base["violations"]
    res["safety_cost"] = tot["safety_cost"] - base["safety_cost"]
    res["ledger"] = ledger
    return res


def _reset_done(env, done):
    """Finished lanes start over; the float32 observation of every lane for the next step.  The device simulators do
    both in ``reset_done`` (one launch in their device mode, the two lines below in their host mode); an environment
    handed in without that method gets the two lines."""
    reset_done = getattr(env, "reset_done", None)
    if reset_done is not None:
        return reset_done(done)
    import torch
    env.reset(done > 0)
    return env.obs.to(torch.float32).clone()


def train_vectorized(agent, env, args, n_steps, log=print, memory=None, check=None, handover=None, episodes=None):
    """Vectorised rollouts: ``env`` is one of ``nlbac_amd.envs.device`` — N environments stepping in
    lock step on the device — and nothing of a transition touches the host: the policy acts on the (N, obs) device
    tensor (one forward for all lanes), the simulator launch writes the next observations / rewards / constraints /
    Lyapunov inputs, the transition rows are assembled in the agent's minibatch layout on the device and appended to a
    ``DeviceReplayMemory`` (which serves both the controller updates and the NODE fit), ``updates_per_step`` updates
    follow every vector step.  The reference's driver is one host environment at a time (``*/main.py::train``,
    restated by ``train`` above and pinned against it); this is the same data flow widened to N lanes, WITHOUT the
    backup-controller hand-over heuristics (which are per-episode host control flow): the primary controller acts in
    every lane.  Time-limit terminations keep mask 1 (U/main.py:150), finished lanes are reset in place by
    ``env.reset_done(done)``, which also hands back the float32 observation of the next step (one launch on an
    environment made with ``device_resets=True``, the torch reset and a float32 copy otherwise).
    ``check``: a callable(step_index, rows) the tests use to look at the rows that were appended.
    Returns dict(steps, updates, episodes, mean_return) — and ``node_validation``, the list of ``NodeValidation``
    records, when ``args.node_validate_every`` is on (every other key keeps its value).

    ``handover``: None / False — the above.  True, or a ``_lib.HandoverParams`` (``vector_handover.params_for``): lane i
    is ``train``'s loop for one environment as far as controllers and replays go (``_train_vectorized_handover``).

    ``episodes``: None / False — the above.  True, a capacity or a ``vector_episodes.EpisodeLedger`` of ``env.n`` lanes:
    one ``push`` per vector step keeps the reference driver's per-episode records on the device (two small launches, no
    host read); the dict gains ``history`` (``train``'s list of per-episode dicts, in log order), ``violations`` and
    ``safety_cost`` (totals over the episodes that finished in this run) and ``ledger``.  Every other key keeps its
    value.  A ledger handed in from an earlier run keeps counting: its own ``records`` / ``totals`` cover its lifetime,
    while ``history``, ``violations`` and ``safety_cost`` are this run's alone (one read of the totals before the first
    step; ``episode`` continues the ledger's numbering, ``total_steps`` and ``updates`` count from this run's start;
    ``safety_cost`` is the difference of two float64 totals; the ledger does not know that a run has ended, so the
    steps of an episode the earlier run left open count toward that lane's first record here — hand the environment on
    with the ledger, or end the earlier run on an episode boundary)."""
    ledger = ledger_base = None
    if episodes is not None and episodes is not False:
        from .vector_episodes import ledger_for
        ledger = ledger_for(episodes, env.n, agent.device)
        ledger_base = _episode_base(ledger)
    if handover is not None and handover is not False:
        return _train_vectorized_handover(agent, env, args, n_steps, log, memory, check, handover, ledger, ledger_base)
    import torch
    from .sac_cbf_clf.replay_memory import DeviceReplayMemory
    dev, lay, N = agent.device, agent.lay, env.n
    barrier = lay.sig is not None
    agent.node_stride = N          # one row per lane per step: a lane's consecutive transitions lie N rows apart
    if memory is None:
        memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    lo = torch.as_tensor(np.asarray(env.action_space.low), dtype=torch.float32, device=dev)
    hi = torch.as_tensor(np.asarray(env.action_space.high), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(args.seed))
    rows = torch.zeros(N, lay.LD, dtype=torch.float32, device=dev)
    obs = env.reset().to(torch.float32).clone()
    ep_ret = torch.zeros(N, dtype=torch.float64, device=dev)
    ret_sum = torch.zeros((), dtype=torch.float64, device=dev)
    n_done = torch.zeros((), dtype=torch.int64, device=dev)
    # (does the task's NODE-fit schedule look at the episode count?  The Pvtol copy's does: tasks.PvtolTask.fit_due)
    from .sac_cbf_clf.tasks import _Task
    needs_episode = type(agent.task).fit_due is not _Task.fit_due
    steps = updates = it = 0
    val = NodeValidation.make(agent, args)
    if getattr(agent, "backup_policy", None) is not None:
        log("vectorised: the backup controller is trained by every update but never acts (the hand-over heuristics are "
            "per-episode host control flow): its replay distribution is the primary controller's, unlike the reference's")
    while steps < n_steps:
        if steps < args.start_steps:
            action = lo + (hi - lo) * torch.rand(N, lay.act_dim, generator=gen, device=dev)
        else:
            action = agent.policy.sample(obs)[0]
        out = env.step(action)
        nobs, reward, constraint = out[:3]
        lya_in, next_lya_in, done = out[-4], out[-3], out[-2]
        if ledger is not None:
            ledger.push(reward, done, out[-1], env.ep_step, int(env.max_episode_steps), vstep=it, updates=updates)
        t = env.ep_step.to(torch.float32)                     # (already advanced by this step)
        timeout = env.ep_step >= int(env.max_episode_steps)
        rows.zero_()
        rows[:, lay.obs:lay.obs + lay.obs_dim] = obs
        rows[:, lay.act:lay.act + lay.act_dim] = action
        rows[:, lay.rew], rows[:, lay.con] = reward.float(), constraint.float()
        if barrier:
            rows[:, lay.sig] = out[3].float()
        rows[:, lay.lya:lay.lya + lay.lya_dim] = lya_in.float()
        rows[:, lay.nlya:lay.nlya + lay.lya_dim] = next_lya_in.float()
        rows[:, lay.nobs:lay.nobs + lay.obs_dim] = nobs.float()
        rows[:, lay.mask] = torch.where(timeout, torch.ones_like(reward), 1.0 - done.to(reward.dtype)).float()
        rows[:, lay.t], rows[:, lay.nt] = t * float(env.dt), (t + 1.0) * float(env.dt)
        memory.push_rows(rows)
        if check is not None:
            check(it, rows)
        ep_ret += reward
        fin = done > 0
        ret_sum += torch.where(fin, ep_ret, torch.zeros_like(ep_ret)).sum()
        n_done += fin.sum()
        ep_ret = torch.where(fin, torch.zeros_like(ep_ret), ep_ret)
        steps += N
        it += 1
        if len(memory) > args.batch_size:
            # the reference driver's trailing argument (P/main.py: the Pvtol copy stops fitting its NODE after episode
            # 100): lanes finish episodes on their own, so the counter is finished episodes per lane, 1-based like the
            # reference's.  Only a task whose fit schedule depends on it pays the scalar read-back (a host sync), and only
            # on the iterations whose update can fit the NODE at all.
            i_episode = None
            if needs_episode and any((updates + k) % args.NODE_model_update_interval == 0 for k in range(args.updates_per_step)):
                i_episode = 1 + int(n_done) // N
            for _ in range(args.updates_per_step):
                if val is not None and val.due(updates):
                    val.run(memory, updates, steps)
                agent.update_parameters(memory, args.batch_size, updates, None, memory, args.NODE_model_update_interval,
                                        i_episode)
                updates += 1
        obs = _reset_done(env, done)                           # (finished lanes start over; the others keep their state)
    torch.cuda.synchronize()
    eps = int(n_done)
    res = dict(steps=steps, updates=updates, episodes=eps, mean_return=float(ret_sum) / max(eps, 1))
    if val is not None:
        res["node_validation"] = val.finish(log)
    if ledger is None:
        log("vectorised: %(steps)d env steps in %(episodes)d finished episodes, %(updates)d updates, mean return %(mean_return).2f" % res)
        return res
    _episode_results(res, ledger, ledger_base, log)
    log("vectorised: %(steps)d env steps in %(episodes)d finished episodes, %(updates)d updates, mean return "
        "%(mean_return).2f, %(violations)d safety violations" % res)
    return res


def _train_vectorized_handover(agent, env, args, n_steps, log, memory, check, handover, ledger=None, ledger_base=None):
    """``train_vectorized`` with the backup-controller hand-over decided per lane on the device
    (``vector_handover.VectorHandover``; DESIGN.md §5 has the definition).  ``memory`` is the NODE replay and receives
    every transition; a ``DeviceKeptReplay`` of the same capacity is the controller replay — it receives the rows of the
    lanes in which the primary controller acted and is what ``update_parameters`` draws its minibatch from.  The action
    of lane i is the backup policy's where ``flags[i]`` is set (the primary policy draws its noise from the global
    generator as without hand-over, the backup policy from a generator of its own), the uniform draw during
    ``start_steps`` either way.  Per vector step, on top of the simulator and the two policies: two launches
    (``nlbac_vector_step_rows``, ``nlbac_ring_append_kept``).  ``check``: callable(step_index, rows, flags) — the rows
    that went into the NODE replay and the flags that decided the step.
    Returns dict(steps, updates, episodes, mean_return, backup_steps).  ``ledger``: the ``episodes=`` ledger; its
    ``backup_steps`` count the flags that decided each step."""
    lay = getattr(agent, "lay", None)
    if getattr(env, "barrier", False) or getattr(lay, "sig", None) is not None:
        raise ValueError("train_vectorized(handover=...): the learned-barrier copies have no backup controller")
    if getattr(agent, "backup_policy", None) is None:
        raise ValueError("train_vectorized(handover=...): this agent has no backup policy to hand over to")
    env_name = getattr(env, "dynamics_mode", None)             # (the barrier copies share their base copy's)
    if env_name not in ("Unicycle", "SimulatedCars", "Pvtol"):
        raise ValueError("train_vectorized(handover=...): no hand-over rules for %r" % (env_name,))
    import torch
    from .sac_cbf_clf.replay_memory import DeviceKeptReplay, DeviceReplayMemory
    from .vector_handover import VectorHandover, params_for
    dev, N = agent.device, env.n
    agent.node_stride = N          # (the NODE replay still holds one row per lane per step)
    if memory is None:
        memory = DeviceReplayMemory(args.replay_size, args.seed, agent, device_rng=True)
    params = params_for(env_name, env) if handover is True else handover
    ho = VectorHandover(env_name, N, dev, params)
    kept = DeviceKeptReplay(memory.capacity, args.seed, agent, draws_from=memory)
    lo = torch.as_tensor(np.asarray(env.action_space.low), dtype=torch.float32, device=dev)
    hi = torch.as_tensor(np.asarray(env.action_space.high), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(args.seed))
    gen_backup = torch.Generator(device=dev)                   # (the backup policy's noise: the global stream, which the
    gen_backup.manual_seed(int(args.seed))                     # primary policy and the updates draw from, does not move)
    obs = env.reset().to(torch.float32).clone()
    ep_ret = torch.zeros(N, dtype=torch.float64, device=dev)
    ret_sum = torch.zeros((), dtype=torch.float64, device=dev)
    n_done = torch.zeros((), dtype=torch.int64, device=dev)
    from .sac_cbf_clf.tasks import _Task
    needs_episode = type(agent.task).fit_due is not _Task.fit_due
    steps = updates = it = 0
    val = NodeValidation.make(agent, args)
    gate_open = False
    log("vectorised: backup-controller hand-over per lane on the device; the controller replay holds the primary "
        "controller's steps only")
    while steps < n_steps:
        if steps < args.start_steps:
            action = lo + (hi - lo) * torch.rand(N, lay.act_dim, generator=gen, device=dev)
        else:
            primary = agent.policy.sample(obs)[0]
            eps = torch.randn(N, lay.act_dim, generator=gen_backup, device=dev)
            action = torch.where(ho.flags[:, None], agent.backup_policy.sample(obs, eps=eps)[0], primary)
        action = action.contiguous()
        decided = ho.flags.clone() if check is not None else None
        out = env.step(action)
        nobs, reward, constraint = out[:3]
        lya_in, next_lya_in, done, info = out[-4], out[-3], out[-2], out[-1]
        info0 = info["reached" if env_name == "SimulatedCars" else "goal_met"]
        if ledger is not None:                                 # (reads the flags that decided the step: ho.push moves them)
            ledger.push(reward, done, info, env.ep_step, int(env.max_episode_steps), flags=ho.flags, vstep=it,
                        updates=updates)
        first = ho.push(memory, kept, obs, action, reward, constraint, lya_in, next_lya_in, nobs, info0, done, env.ep_step,
                        float(env.dt), int(env.max_episode_steps))
        if check is not None:
            idx = (first + torch.arange(N, device=dev)) % memory.capacity
            check(it, memory.rows[idx], decided)
        ep_ret += reward
        fin = done > 0
        ret_sum += torch.where(fin, ep_ret, torch.zeros_like(ep_ret)).sum()
        n_done += fin.sum()
        ep_ret = torch.where(fin, torch.zeros_like(ep_ret), ep_ret)
        steps += N
        it += 1
        if not gate_open:                                      # (the only host read of the run, until it has passed)
            gate_open = kept.refresh_len() > args.batch_size
        if gate_open:
            i_episode = None                                   # (as without hand-over)
            if needs_episode and any((updates + k) % args.NODE_model_update_interval == 0 for k in range(args.updates_per_step)):
                i_episode = 1 + int(n_done) // N
            for _ in range(args.updates_per_step):
                if val is not None and val.due(updates):
                    val.run(memory, updates, steps)
                agent.update_parameters(kept, args.batch_size, updates, None, memory, args.NODE_model_update_interval,
                                        i_episode)
                updates += 1
        obs = _reset_done(env, done)
    torch.cuda.synchronize()
    eps_n = int(n_done)
    res = dict(steps=steps, updates=updates, episodes=eps_n, mean_return=float(ret_sum) / max(eps_n, 1),
               backup_steps=ho.backup_steps())
    if val is not None:
        res["node_validation"] = val.finish(log)
    if ledger is None:
        log("vectorised: %(steps)d env steps in %(episodes)d finished episodes, %(updates)d updates, mean return "
            "%(mean_return).2f, %(backup_steps)d steps under the backup controller" % res)
        return res
    _episode_results(res, ledger, ledger_base, log)
    log("vectorised: %(steps)d env steps in %(episodes)d finished episodes, %(updates)d updates, mean return "
        "%(mean_return).2f, %(backup_steps)d steps under the backup controller, %(violations)d safety violations" % res)
    return res


def evaluate_vectorized(agent, env, episodes_per_lane=1, ledger=None):
    """Evaluation of the acting policy on the device simulators, the reference's ``select_action(evaluate=True)`` for
    every lane of ``env``: the action is the policy's mean (``policy.sample(obs, eps=zeros)[2]``), there are no updates
    and no replay, finished lanes are reset in place and a ``vector_episodes.EpisodeLedger`` records every episode.
    Runs until every lane has finished ``episodes_per_lane`` episodes — at most ``episodes_per_lane *
    max_episode_steps`` vector steps.

    Host reads.  A lane that has finished is reset and keeps writing records, one per episode, so short episodes fill
    the ring fast: a vector step writes up to N records.  The new records are therefore read every ``capacity // N``
    vector steps (and at the time limit), which no run of episodes can overflow, and the same read tells whether every
    lane has its ``episodes_per_lane`` — the run stops at the first read that finds so, at most ``capacity // N - 1``
    steps late.  ``lane_episodes`` itself is read once, before the first step.  The default ledger holds ``min(64 N,
    2^20)`` records (at least ``max(4 N, 4096)``): a read every 64 vector steps up to 16 384 lanes.

    Draws nothing from torch's global generators and changes no agent state: a training run on the Unicycle / Pvtol
    simulators that evaluates in between continues bit for bit.  (A host-mode ``DeviceSimulatedCarsEnv`` draws its
    initial velocity noise from numpy's global generator: evaluating on it moves that stream, here as anywhere.  One
    made with ``device_resets=True`` draws on the device from its own counters, and then this call draws nothing from
    any global generator, numpy's included.)  ``env`` is reset first and left wherever the last step took it; finished
    lanes are restarted by ``env.reset_done`` (one launch on a device-mode environment).

    Returns dict(history, arrays, episodes, steps, mean_return, std_return, mean_length, std_length,
    violations_per_episode, safety_cost_per_episode, goal_rate, timeout_rate): the first ``episodes_per_lane`` records of
    every lane in log order (list of dicts / numpy arrays, ``EpisodeLedger.records``) and their summary."""
    if isinstance(episodes_per_lane, bool) or not isinstance(episodes_per_lane, (int, np.integer)) or episodes_per_lane < 1:
        raise ValueError("evaluate_vectorized: episodes_per_lane is an int of at least 1 (got %r)" % (episodes_per_lane,))
    from .vector_episodes import EpisodeLedger, history_of, ledger_for
    N, max_steps, per_lane = int(env.n), int(env.max_episode_steps), int(episodes_per_lane)
    if max_steps < 1:
        raise ValueError("evaluate_vectorized: the environment's max_episode_steps must be at least 1")
    if ledger is None:
        ledger = EpisodeLedger(N, agent.device, capacity=max(4 * N, 4096, min(64 * N, 1 << 20)))
    else:
        ledger = ledger_for(ledger, N, agent.device)
    import torch
    dev = agent.device
    obs = env.reset().to(torch.float32).clone()
    zeros = torch.zeros(N, agent.lay.act_dim, dtype=torch.float32, device=dev)
    seen = int(ledger.totals()["episodes"]) if ledger.pushes else 0      # (a ledger handed in may hold records already)
    base = ledger.lane_episodes.cpu().numpy().astype(np.int64)
    read_every = ledger.capacity // N              # (>= 1; the records of that many steps cannot overflow the ring)
    parts, have, it, last, limit = [], 0, 0, 0, per_lane * max_steps
    while it < limit and have < N * per_lane:
        with torch.no_grad():
            action = agent.policy.sample(obs, eps=zeros)[2].contiguous()
        out = env.step(action)
        ledger.push(out[1], out[-2], out[-1], env.ep_step, max_steps, vstep=it, updates=0)
        obs = _reset_done(env, out[-2])
        it += 1
        if it - last >= read_every or it == limit:
            arrays = ledger.arrays(since=seen)
            seen, last = arrays.pop("total"), it
            keep = arrays["lane_episode"] - base[arrays["lane"]] < per_lane     # (a lane's later episodes are dropped)
            parts.append({k: v[keep] for k, v in arrays.items()})
            have += int(keep.sum())
    arrays = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    assert have == len(arrays["episode"]) == N * per_lane, \
        "evaluate_vectorized: %d records for %d lanes x %d episodes" % (have, N, per_lane)
    ret, length = arrays["reward"], arrays["length"].astype(np.float64)
    return dict(history=history_of(arrays), arrays=arrays, episodes=have, steps=it * N,
                mean_return=float(ret.mean()), std_return=float(ret.std()), mean_length=float(length.mean()),
                std_length=float(length.std()), violations_per_episode=float(arrays["violations"].mean()),
                safety_cost_per_episode=float(arrays["safety_cost"].mean()), goal_rate=float(arrays["goal_met"].mean()),
                timeout_rate=float(arrays["timeout"].mean()))


def main(argv=None):
    args = get_args(argv)
    import nlbac_amd  # noqa: F401
    from . import envs
    barrier = has_barrier_signal(args.env)
    if barrier:
        from .neural_barrier_certificate.sac_cbf_clf.sac_cbf_clf import SAC_CBF_CLF
        from .neural_barrier_certificate.sac_cbf_clf.replay_memory import DeviceReplayMemory, ReplayMemory
    else:
        from .sac_cbf_clf.sac_cbf_clf import SAC_CBF_CLF
        from .sac_cbf_clf.replay_memory import DeviceReplayMemory, ReplayMemory
    from .sac_cbf_clf.dynamics import DynamicsModel
    env = envs.make(args.env, args.seed)
    if args.seed >= 0:       # U/main.py:253-258: every generator is seeded before the agent (and its networks) exist
        import random
        import torch
        env.seed(args.seed)
        random.seed(args.seed)
        env.action_space.seed(args.seed)
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
    agent = SAC_CBF_CLF(env.observation_space.shape[0], env.action_space, env, args)
    agent.use_graphs = bool(args.hipgraphs)
    agent.solver = args.solver
    if args.vector_envs > 0:
        from .envs import device as device_envs
        args.replay_size = min(args.replay_size, 1 << 20)
        if args.vector_episode_tsv and args.vector_episodes is None:
            args.vector_episodes = True
        # (SimulatedCars has one vectorised form: its host-mode reset is a per-lane host loop over numpy's global stream)
        device_resets = bool(args.vector_device_resets) or args.env == "SimulatedCars"
        venv = device_envs.make(args.env, args.vector_envs, seed=max(args.seed, 0),
                                **vector_env_options(args.env, device_resets, args.vector_init_spread))
        res = train_vectorized(agent, venv, args, args.max_steps or 100000, handover=args.vector_handover or None,
                               episodes=args.vector_episodes)
        if args.vector_episode_tsv:
            from .vector_episodes import write_tsv
            write_tsv(args.vector_episode_tsv, res["history"])
        return res
    dynamics_model = DynamicsModel(env, args)
    if args.device_replay:
        cap = min(args.replay_size, 1 << 20)
        memory = DeviceReplayMemory(cap, args.seed, agent, device_rng=args.device_rng)
        node_memory = DeviceReplayMemory(cap, args.seed + 1 if args.device_rng else args.seed, agent,
                                         device_rng=args.device_rng)
    else:
        memory, node_memory = ReplayMemory(args.replay_size, args.seed), ReplayMemory(args.replay_size, args.seed)
    return train(agent, env, dynamics_model, args, memory, node_memory)


if __name__ == "__main__":
    main()
