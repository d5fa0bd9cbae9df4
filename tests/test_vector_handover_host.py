"""Host side of the vectorised driver's backup-controller hand-over (``nlbac_amd.vector_handover``,
``train.train_vectorized(handover=...)``): the C ABI declares and the binding binds the three entry points and the
parameter struct, the struct is filled from the host classes' attributes (the constants live in ``train.py`` alone), the
option parses, and what cannot hand over says so before anything touches a device.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from nlbac_amd import _lib, train, vector_handover
from nlbac_amd.sac_cbf_clf.replay_memory import DeviceKeptReplay, DeviceReplayMemory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nlbac_vector_step_rows", "nlbac_ring_append_kept", "nlbac_sample_rows_head")


def header():
    return open(os.path.join(ROOT, "include", "nlbac_hip.h")).read()


def test_header_declares_the_entry_points_and_the_struct_and_the_abi_stays_17():
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, txt), "%s is not declared" % name
    assert re.search(r"typedef struct nlbac_handover_params\s*\{.*?\}\s*nlbac_handover_params;", txt, flags=re.S)
    assert int(re.search(r"#define NLBAC_ABI_VERSION (\d+)", txt).group(1)) == 17 == _lib.ABI_VERSION
    assert "handover_kernels.hip" in open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()


def test_binding_binds_them_and_its_structs_match_the_header(tmp_path):
    _lib.build()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.nlbac_abi_version() == 17
    pairs = [("nlbac_handover_params", _lib.HandoverParams, "operator_dist"), ("nlbac_row_layout", _lib.RowLayout, "nt")]
    body = "".join('printf("%%zu %%zu\\n", sizeof(%s), offsetof(%s, %s));' % (c, c, last) for c, _, last in pairs)
    body += 'printf("%d %d\\n", NLBAC_HANDOVER_RING, NLBAC_HANDOVER_ISTATE);'
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlbac_hip.h"\nint main(void){%s return 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    for k, (cname, cls, last) in enumerate(pairs):
        assert (C.sizeof(cls), getattr(cls, last).offset) == (out[2 * k], out[2 * k + 1]), cname
    assert (_lib.HANDOVER_RING, _lib.HANDOVER_ISTATE) == (out[4], out[5])
    # every member of the C struct is bound, in order
    members = re.search(r"typedef struct nlbac_handover_params\s*\{(.*?)\}", re.sub(r"/\*.*?\*/", "", header(), flags=re.S),
                        flags=re.S).group(1)
    assert re.findall(r"(?:int|double)\s+(\w+);", members) == [f[0] for f in _lib.HandoverParams._fields_]


def test_params_for_reproduces_every_constant_of_the_host_classes():
    U, Cc, P = train._UnicycleHandover, train._CarsHandover, train._PvtolHandover
    # the values the reference's drivers use (U/main.py:39-142, C/main.py:41-112, P/main.py:40-200)
    assert (U.first_backup_episode, U.STUCK2, U.CHECKS, U.MAX_BACKUP, U.AWAY2) == (4, 0.01, 8, 30, 0.6)
    assert (Cc.first_backup_episode, Cc.memory_t_shift, Cc.GAP, Cc.MAX_BACKUP, Cc.MIN_BACKUP) == (0, -1, 2.5, 15, 5)
    assert (P.first_backup_episode, P.STUCK2, P.CHECKS, P.MAX_BACKUP, P.AWAY2) == (3, 0.015, 8, 30, 1.0)
    assert (P.RUN_CHECKS, P.RUN_MAX_BACKUP, P.BACK_FRAC, P.X_MID) == (1, 15, 0.9, 4.5)
    assert (train._Handover.MIN_CHECK_STEP, train._Handover.LOOKBACK) == (50, 40)
    p = vector_handover.params_for("Unicycle")
    assert (p.kind, p.first_backup_episode, p.min_check_step, p.lookback, p.memory_t_shift) == (0, 4, 50, 40, 0)
    assert (p.stuck2, p.checks, p.max_backup, p.away2) == (U.STUCK2, U.CHECKS, U.MAX_BACKUP, U.AWAY2)
    p = vector_handover.params_for("SimulatedCars")
    assert (p.kind, p.first_backup_episode, p.memory_t_shift) == (1, 0, -1)
    assert (p.gap, p.max_backup, p.min_backup) == (Cc.GAP, Cc.MAX_BACKUP, Cc.MIN_BACKUP)
    env = types.SimpleNamespace(operator_dist=1.25)
    p = vector_handover.params_for("Pvtol", env)
    assert (p.kind, p.first_backup_episode, p.min_check_step, p.lookback, p.memory_t_shift) == (2, 3, 50, 40, 0)
    assert (p.stuck2, p.checks, p.max_backup, p.away2) == (P.STUCK2, P.CHECKS, P.MAX_BACKUP, P.AWAY2)
    assert (p.run_checks, p.run_max_backup, p.back_frac, p.x_mid, p.operator_dist) == (1, 15, 0.9, 4.5, 1.25)
    assert vector_handover.params_for("Pvtol", env, first_backup_episode=2 ** 30).first_backup_episode == 2 ** 30
    with pytest.raises(ValueError):
        vector_handover.params_for("Pvtol")                       # operator_dist is one of the thresholds
    with pytest.raises(ValueError):
        vector_handover.params_for("UnicycleBarrier")
    with pytest.raises(ValueError):
        vector_handover.params_for("Unicycle", no_such_field=1)
    # a changed class attribute reaches the struct: the constants live in one place
    old = U.CHECKS
    try:
        U.CHECKS = 11
        assert vector_handover.params_for("Unicycle").checks == 11
    finally:
        U.CHECKS = old


def test_host_classes_behave_as_before_the_literals_became_attributes():
    """A hand-written trace through every branch of ``_CarsHandover`` (the class whose literals were lifted and that no
    simulator trace reaches): hand-over on a close approach with ``reached``, the 15-step cap, the early return."""
    ho = train._CarsHandover(None)
    ho.begin_episode(0)
    obs = lambda d34, d45: [0, 0, 0, 0, (d34 + d45) / 100.0, 0, d45 / 100.0, 0, 0.0, 0]
    ho.after_step(1, None, None, obs(5.0, 2.0), {"reached": 0})
    assert not ho.use_backup
    ho.after_step(2, None, None, obs(5.0, 2.0), {"reached": 1})
    assert ho.use_backup
    for k in range(5):
        ho.on_backup_action()
        ho.after_step(3 + k, None, None, obs(5.0, 2.0), {"reached": 1})
    assert ho.use_backup and ho.backup_time == 5
    ho.after_step(8, None, None, obs(5.0, 3.0), {"reached": 1})   # both gaps open after 5 steps: back
    assert not ho.use_backup
    ho.after_step(9, None, None, obs(5.0, 2.0), {"reached": 1})
    for k in range(15):
        assert ho.use_backup
        ho.on_backup_action()
        ho.after_step(10 + k, None, None, obs(1.0, 2.0), {"reached": 1})
    assert not ho.use_backup                                       # the cap


def test_the_option_parses():
    assert train.get_args(["--vector_envs", "8", "--vector_handover"]).vector_handover is True
    assert train.get_args(["--vector_envs", "8"]).vector_handover is False


class _NoDevice:
    """An agent / environment stand-in whose device would raise if anything reached for it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        raise AssertionError("train_vectorized touched %r before refusing the hand-over" % name)


def test_handover_is_refused_where_there_is_no_backup_controller():
    args = types.SimpleNamespace(replay_size=64, seed=0, start_steps=0, batch_size=4, updates_per_step=1,
                                 NODE_model_update_interval=10)
    barrier_env = _NoDevice(barrier=True)
    agent = _NoDevice(lay=types.SimpleNamespace(sig=4), backup_policy=object())
    with pytest.raises(ValueError, match="barrier"):
        train.train_vectorized(agent, barrier_env, args, 16, handover=True)
    agent = _NoDevice(lay=types.SimpleNamespace(sig=None), backup_policy=None)
    with pytest.raises(ValueError, match="backup policy"):
        train.train_vectorized(agent, _NoDevice(barrier=False), args, 16, handover=True)
    with pytest.raises(ValueError, match="backup policy"):
        train.train_vectorized(agent, _NoDevice(barrier=False), args, 16,
                               handover=vector_handover.params_for("Unicycle"))


def test_kept_replay_has_no_host_draw():
    kept = DeviceKeptReplay.__new__(DeviceKeptReplay)             # (no device: the constructor allocates the ring)
    with pytest.raises(NotImplementedError, match="device"):
        kept.sample(4)
    assert not hasattr(DeviceKeptReplay, "push") and DeviceKeptReplay.device_rng is True
    assert callable(DeviceReplayMemory.reserve_rows)
