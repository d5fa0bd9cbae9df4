"""GPU: throughput of the vectorised driver (train.train_vectorized): N device environments + one update per vector step.

    python tools/vector_rate.py [N [B]] [--env=NAME] [--device-resets] [--init-spread=SX,SY] [--handover] [--episodes]
                                [--launches] [--iters=K] [--node-validate-every=K]

``--env=NAME``: Unicycle (default), Pvtol, SimulatedCars (which always resets on the device) or QuadrotorLike.
``--device-resets``: environments made with ``device_resets=True`` — finished lanes restart by one launch per vector step
(``nlbac_env_reset_rows`` / ``nlbac_cars_env_reset``) instead of torch ops with host syncs.
``--init-spread=SX,SY``: environments made with ``init_spread=(SX, SY)`` — every restart draws its start position in that
launch (``nlbac_unicycle_env_reset`` / ``nlbac_pvtol_env_reset`` / ``nlbac_quadrotor_env_reset``); implies ``--device-resets``.

``--handover``: with the backup-controller hand-over decided per lane on the device (two replays, two acting policies).
``--episodes``: with the per-episode ledger on the device (``episodes=True``: two more launches per vector step).
``--launches``: after the timed run, a short run that counts the library's launches (``_lib.call``) per vector step.
``--node-validate-every=K``: with the NODE validated on 4096 windows of 3 steps before every K-th update
(``args.node_validate_every``; read at the end of the run).
``--iters=K``: vector steps of the timed run (300; a kernel trace of two run lengths, differenced, counts the kernels of
a vector step)."""
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import nlbac_amd
from nlbac_amd.envs import device as denv
from nlbac_amd.train import train_vectorized
from test_agent_parity_gpu import make_agent

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
handover, launches, episodes = "--handover" in sys.argv, "--launches" in sys.argv, "--episodes" in sys.argv
N, B, iters = int(argv[0]) if len(argv) > 0 else 4096, int(argv[1]) if len(argv) > 1 else 4096, 300
iters = next((int(a[8:]) for a in sys.argv[1:] if a.startswith("--iters=")), iters)
name = next((a[6:] for a in sys.argv[1:] if a.startswith("--env=")), "Unicycle")
if name not in ("Unicycle", "Pvtol", "SimulatedCars", "QuadrotorLike"):
    sys.exit("--env=NAME: Unicycle, Pvtol, SimulatedCars or QuadrotorLike (got %r)" % name)
spread = next((tuple(float(v) for v in a[14:].split(",")) for a in sys.argv[1:] if a.startswith("--init-spread=")), None)
device_resets = "--device-resets" in sys.argv or name == "SimulatedCars" or spread is not None
env_kw = {"init_spread": spread} if spread is not None else {}
make_env = lambda seed: denv.make(name, N, seed=seed, device_resets=device_resets, **env_kw)
agent, _ = make_agent(B, 256, 0, "dopri5", name, {"Unicycle": 50.0, "Pvtol": 0.8, "QuadrotorLike": 1.0}.get(name))
env = make_env(0)
args = types.SimpleNamespace(replay_size=1 << 20, seed=0, start_steps=2 * N, batch_size=B, updates_per_step=1,
                             NODE_model_update_interval=10)
validate = next((int(a[22:]) for a in sys.argv[1:] if a.startswith("--node-validate-every=")), 0)
if validate:
    args.node_validate_every = validate
kw = {"handover": True} if handover else {}
if episodes:
    kw["episodes"] = True
train_vectorized(agent, env, args, 20 * N, log=lambda *a: None, **kw)        # warm-up (allocations, first launches)
torch.cuda.synchronize(); t0 = time.perf_counter()
res = train_vectorized(agent, make_env(1), args, iters * N, log=lambda *a: None, **kw)
dt = time.perf_counter() - t0
print("%s, N=%d lanes, batch %d, resets on the %s%s%s%s%s: %d env steps + %d updates in %.3f s = %.2f M env steps/s, %.2f ms per vector step"
      % (name, N, B, "device" if device_resets else "host", ", start spread %g, %g" % spread if spread is not None else "",
         ", hand-over on (%d backup steps)" % res["backup_steps"] if handover else "",
         ", ledger on (%d records, %d safety violations)" % (len(res["history"]), res["violations"]) if episodes else "",
         ", NODE validated every %d updates (%d records)" % (validate, len(res["node_validation"])) if validate else "",
         res["steps"], res["updates"], dt, res["steps"] / dt / 1e6, 1e3 * dt / iters))
if launches:
    from nlbac_amd import _lib
    names, real, n_it = [], _lib.call, 40
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    marks = []
    train_vectorized(agent, make_env(2), args, n_it * N, log=lambda *a: None,
                     check=lambda it, *a: marks.append(len(names)), **kw)
    _lib.call = real
    per_step = [marks[k + 1] - marks[k] for k in range(10, n_it - 1)]         # (past the warm-up and the gate)
    own = names[marks[20]:marks[21]]
    driver = [n for n in own if n.endswith("_env_step") or n in (
        "nlbac_vector_step_rows", "nlbac_ring_append_kept", "nlbac_episode_step", "nlbac_episode_append",
        "nlbac_env_reset_rows", "nlbac_cars_env_reset", "nlbac_quadrotor_env_reset", "nlbac_unicycle_env_reset",
        "nlbac_pvtol_env_reset")]
    print("library launches per vector step (update included): min %d max %d; the driver's own: %s"
          % (min(per_step), max(per_step), ", ".join(driver)))
