"""Host-side checks of the vectorised driver's episode ledger (``nlbac_amd.vector_episodes``; no GPU needed): every
refusal of ``EpisodeLedger`` and of ``train_vectorized(episodes=...)`` comes before anything touches a device — with
every device entry patched to fail, as ``test_odeint_dense_tile_host`` patches them — the record layout is the
header's, and the two ``nlbac_episode_*`` entry points refuse bad arguments with a message before anything is launched
(every pointer handed over is host memory that a refused call never touches)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Every way to a device fails: a check that came late shows as an AssertionError instead of the error it should
    have raised."""
    from nlbac_amd import _lib

    def fail(*a, **k):
        raise AssertionError("a check came after the first device call")
    monkeypatch.setattr(_lib, "call", fail)
    monkeypatch.setattr(_lib, "load", fail)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", fail)
    monkeypatch.setattr(torch.cuda, "current_stream", fail)


# ---------------------------------------------------------------------------------------------------------------------
# EpisodeLedger
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, -1, 65537, 2.0, "8", True, None])
def test_lanes_are_an_int_between_1_and_65536(n, no_device):
    from nlbac_amd.vector_episodes import EpisodeLedger
    with pytest.raises(ValueError, match="65536"):
        EpisodeLedger(n, "cuda")


@pytest.mark.parametrize("n,capacity", [(8, 7), (600, 599), (8, 0), (8, -4), (8, 16.0), (8, True)])
def test_capacity_is_an_int_of_at_least_n(n, capacity, no_device):
    from nlbac_amd.vector_episodes import EpisodeLedger
    with pytest.raises(ValueError, match="capacity"):
        EpisodeLedger(n, "cuda", capacity=capacity)


def test_default_capacity_and_the_state_a_ledger_starts_with(no_device):
    from nlbac_amd.vector_episodes import EpisodeLedger
    assert EpisodeLedger(8, "cpu").capacity == 4096 and EpisodeLedger(2000, "cpu").capacity == 8000
    led = EpisodeLedger(8, "cpu", capacity=8)
    assert led.capacity == 8 and led.half == 0 and led.head.tolist() == [[0, 0], [0, 0]]
    assert led.lane_episodes.dtype == torch.int32 and led.lane_episodes.tolist() == [0] * 8
    assert led._ring.data_ptr() % 16 == 0 and led._ring.numel() * 8 == 8 * 64


def step_inputs(n=8, **over):
    kw = dict(reward=torch.zeros(n, dtype=torch.float64), done=torch.zeros(n, dtype=torch.int32),
              info=torch.zeros(n, 3, dtype=torch.float64), ep_step=torch.ones(n, dtype=torch.int32), max_episode_steps=20)
    kw.update(over)
    return kw


BAD_PUSHES = [
    ("reward", dict(reward=torch.zeros(8, dtype=torch.float32))),
    ("reward", dict(reward=torch.zeros(9, dtype=torch.float64))),
    ("reward", dict(reward=torch.zeros(8, 1, dtype=torch.float64))),
    ("reward", dict(reward=torch.zeros(8, 2, dtype=torch.float64)[:, 0])),
    ("reward", dict(reward=np.zeros(8))),
    ("done", dict(done=torch.zeros(8, dtype=torch.bool))),
    ("done", dict(done=torch.zeros(8, dtype=torch.int64))),
    ("done", dict(done=torch.zeros(8, dtype=torch.float32))),
    ("done", dict(done=torch.zeros(7, dtype=torch.int32))),
    ("ep_step", dict(ep_step=torch.ones(8, dtype=torch.int64))),
    ("ep_step", dict(ep_step=torch.ones(16, dtype=torch.int32)[::2])),
    ("info", dict(info=torch.zeros(8, 3, dtype=torch.float32))),
    ("info", dict(info=torch.zeros(8, 2, dtype=torch.float64))),
    ("info", dict(info=torch.zeros(8, dtype=torch.float64))),
    ("info", dict(info=torch.zeros(3, 8, dtype=torch.float64).t())),
    ("info", dict(info=torch.zeros(8, 4, dtype=torch.float64), first_key_column=2)),
    ("info", dict(info={"goal_met": torch.zeros(8, dtype=torch.float64), "num_safety_violation": torch.zeros(8, dtype=torch.float64),
                        "safety_cost": torch.zeros(8, dtype=torch.float64)})),
    ("info", dict(info={"goal_met": torch.zeros(8, 3, dtype=torch.float64)[:, 0]})),
    ("first_key_column", dict(first_key_column=-1)),
    ("flags", dict(flags=torch.zeros(8, dtype=torch.int32))),
    ("flags", dict(flags=torch.zeros(9, dtype=torch.bool))),
    ("max_episode_steps", dict(max_episode_steps=0)),
    ("max_episode_steps", dict(max_episode_steps=20.0)),
    ("vstep", dict(vstep=-1)),
    ("vstep", dict(vstep=2 ** 31)),
    ("updates", dict(updates=-1)),
    ("updates", dict(updates=1.5)),
]


@pytest.mark.parametrize("what,over", BAD_PUSHES, ids=["%s-%d" % (w, j) for j, (w, _) in enumerate(BAD_PUSHES)])
def test_push_refuses_wrong_dtypes_and_shapes(what, over, no_device):
    from nlbac_amd.vector_episodes import EpisodeLedger
    led = EpisodeLedger(8, "cpu")
    kw = dict(step_inputs(), vstep=0, updates=0)
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        led.push(**kw)
    assert led.pushes == 0 and led.half == 0


def test_push_takes_the_simulators_info_dict_and_gets_as_far_as_the_device_check(no_device):
    """With everything in order — the info dict as ``envs.device`` returns it, or a wider block with
    ``first_key_column`` — a CPU ledger is refused last, by the device check, and no further."""
    from nlbac_amd.vector_episodes import EpisodeLedger
    led = EpisodeLedger(8, "cpu")
    block = torch.zeros(8, 3, dtype=torch.float64)
    info = {"goal_met": block[:, 0], "num_safety_violation": block[:, 1], "safety_cost": block[:, 2]}
    wide = torch.zeros(8, 5, dtype=torch.float64)
    for kw in (step_inputs(info=info), step_inputs(info=wide, first_key_column=2),
               step_inputs(flags=torch.zeros(8, dtype=torch.bool)), step_inputs(flags=torch.zeros(8, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="CUDA"):
            led.push(**kw, vstep=3, updates=7)
    assert led._info0(info, 0)[1:] == (block.data_ptr(), 3)
    assert led._info0(wide, 2)[1:] == (wide.data_ptr() + 16, 5)


def test_records_and_totals_of_an_empty_ledger(no_device):
    from nlbac_amd.vector_episodes import HISTORY_KEYS, EpisodeLedger
    led = EpisodeLedger(8, "cpu")
    arrays, history = led.records()
    assert history == [] and arrays["total"] == 0 and all(len(arrays[k]) == 0 for k in HISTORY_KEYS)
    assert set(led.totals().values()) == {0}
    with pytest.raises(ValueError, match="since"):
        led.records(since=1)
    with pytest.raises(ValueError, match="since"):
        led.records(since=-1)


def test_records_decode_the_ring_in_log_order_and_name_capacity_when_overwritten(no_device):
    """A ring filled on the host, record k in slot k mod capacity: the decoding, the history's keys and types, and the
    refusal of a ``since`` the ring no longer holds."""
    from nlbac_amd.vector_episodes import HISTORY_KEYS, RECORD_DTYPE, EpisodeLedger
    n, cap, total = 4, 6, 15
    led = EpisodeLedger(n, "cpu", capacity=cap)
    ring = np.zeros(cap, dtype=RECORD_DTYPE)
    for k in range(total):
        ring[k % cap] = (0.5 * k, 0.25 * k, k % 3, float(k % 2), 10 + k, k % n, k // n, k // 2, 7 * k, (k + 1) % 2, k % 5, 0)
    led._ring.copy_(torch.from_numpy(ring.view(np.int64)))
    led.half = 1
    led.head[1, 0], led.head[1, 1] = total % cap, total
    arrays, history = led.records(since=total - cap)
    ks = np.arange(total - cap, total)
    assert arrays["total"] == total and arrays["episode"].tolist() == ks.tolist()
    assert arrays["reward"].tolist() == (0.5 * ks).tolist() and arrays["safety_cost"].tolist() == (0.25 * ks).tolist()
    assert arrays["violations"].tolist() == (ks % 3).tolist() and arrays["goal_met"].tolist() == (ks % 2).tolist()
    assert arrays["length"].tolist() == (10 + ks).tolist() and arrays["lane"].tolist() == (ks % n).tolist()
    assert arrays["lane_episode"].tolist() == (ks // n).tolist() and arrays["total_steps"].tolist() == ((ks // 2 + 1) * n).tolist()
    assert arrays["updates"].tolist() == (7 * ks).tolist() and arrays["timeout"].tolist() == ((ks + 1) % 2).tolist()
    assert arrays["backup_steps"].tolist() == (ks % 5).tolist()
    assert [tuple(h) for h in history] == [HISTORY_KEYS] * cap
    assert history[0] == dict(episode=9, reward=4.5, length=19, violations=0, safety_cost=2.25, goal_met=1, timeout=0,
                              lane=1, lane_episode=2, total_steps=20, updates=63, backup_steps=4)
    assert all(type(history[0][k]) is (float if k in ("reward", "safety_cost") else int) for k in HISTORY_KEYS)
    assert led.records(since=total)[1] == [] and len(led.records(since=total - 1)[1]) == 1
    for since in (0, total - cap - 1):
        with pytest.raises(ValueError, match="capacity"):
            led.records(since=since)


def test_the_record_layout_is_the_headers(tmp_path):
    """``RECORD_DTYPE`` / ``_lib.EpisodeRecord`` against the struct of include/nlbac_hip.h as gcc lays it out."""
    from nlbac_amd import _lib
    from nlbac_amd.vector_episodes import RECORD_DTYPE
    names = [f[0] for f in _lib.EpisodeRecord._fields_]
    assert names == list(RECORD_DTYPE.names)
    body = 'printf("%zu %zu\\n", sizeof(nlbac_episode_record), _Alignof(nlbac_episode_record));' + "".join(
        'printf("%s %%zu\\n", offsetof(nlbac_episode_record, %s));' % (f, f) for f in names)
    body += 'printf("%d %d\\n", NLBAC_EPISODE_DSTATE, NLBAC_EPISODE_ISTATE);'
    src, exe = tmp_path / "rec.c", tmp_path / "rec"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlbac_hip.h"\nint main(void){%s return 0;}\n' % body)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0] == "64 16"
    for line, f in zip(out[1:], names):
        assert line == "%s %d" % (f, RECORD_DTYPE.fields[f][1]) == "%s %d" % (f, getattr(_lib.EpisodeRecord, f).offset)
    assert out[1 + len(names)] == "%d %d" % (_lib.EPISODE_DSTATE, _lib.EPISODE_ISTATE)


# ---------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handover", [None, True])
def test_train_vectorized_refuses_a_ledger_of_another_width(handover, no_device):
    from nlbac_amd.train import train_vectorized
    from nlbac_amd.vector_episodes import EpisodeLedger
    agent, env = types.SimpleNamespace(device=torch.device("cpu")), types.SimpleNamespace(n=16)
    with pytest.raises(ValueError, match="8 lanes, the environment 16"):
        train_vectorized(agent, env, None, 100, handover=handover, episodes=EpisodeLedger(8, "cpu"))
    for bad in ("yes", 2.5, [4096]):
        with pytest.raises(ValueError, match="episodes="):
            train_vectorized(agent, env, None, 100, handover=handover, episodes=bad)
    with pytest.raises(ValueError, match="capacity"):
        train_vectorized(agent, env, None, 100, handover=handover, episodes=15)


def test_evaluate_vectorized_checks_its_arguments_first(no_device):
    from nlbac_amd.train import evaluate_vectorized
    from nlbac_amd.vector_episodes import EpisodeLedger
    agent, env = types.SimpleNamespace(device=torch.device("cpu")), types.SimpleNamespace(n=16, max_episode_steps=20)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="episodes_per_lane"):
            evaluate_vectorized(agent, env, bad)
    with pytest.raises(ValueError, match="8 lanes, the environment 16"):
        evaluate_vectorized(agent, env, 1, ledger=EpisodeLedger(8, "cpu"))


def test_command_line_options():
    from nlbac_amd.train import get_args
    assert get_args([]).vector_episodes is None and get_args([]).vector_episode_tsv is None
    assert get_args(["--vector_episodes"]).vector_episodes is True
    assert get_args(["--vector_episodes", "9000"]).vector_episodes == 9000
    assert get_args(["--vector_episode_tsv", "log.tsv"]).vector_episode_tsv == "log.tsv"


def test_tsv_has_a_header_and_one_line_per_record(tmp_path):
    from nlbac_amd.vector_episodes import HISTORY_KEYS, write_tsv
    rec = dict(episode=0, reward=-1.25, length=20, violations=3, safety_cost=0.1, goal_met=0, timeout=1, lane=5,
               lane_episode=0, total_steps=1280, updates=12, backup_steps=0)
    path = tmp_path / "log.tsv"
    write_tsv(str(path), [rec, dict(rec, episode=1, lane=6)])
    lines = path.read_text().split("\n")
    assert lines[0].split("\t") == list(HISTORY_KEYS) and len(lines) == 4 and lines[3] == ""
    assert lines[1].split("\t") == ["0", "-1.25", "20", "3", "0.10000000000000001", "0", "1", "5", "0", "1280", "12", "0"]
    assert float(lines[1].split("\t")[4]) == 0.1 and lines[2].split("\t")[7] == "6"


# ---------------------------------------------------------------------------------------------------------------------
# the C entries: one argument changed per case from a call that would launch
# ---------------------------------------------------------------------------------------------------------------------
def step_args():
    host = (C.c_double * 64)()
    p = C.addressof(host)
    return dict(n=8, reward=p, info0=p, info_ld=3, done=p, ep_step=p, max_steps=20, flags=None, dstate=p, istate=p, fin=p,
                counts=p, s=None), host


def append_args():
    host = (C.c_double * 64)()
    p = (C.addressof(host) + 15) // 16 * 16                 # (the ring: aligned to 16 bytes)
    return dict(n=8, fin=p, counts=p, dstate=p, istate=p, ring=p, capacity=8, head=p, half=0, vstep=0, updates=0, s=None), host


STEP_REFUSALS = [(dict(**{k: None}), "null") for k in ("reward", "info0", "done", "ep_step", "dstate", "istate", "fin", "counts")] + [
    (dict(n=0), "65536"), (dict(n=-3), "65536"), (dict(n=65537), "65536"), (dict(info_ld=2), "info_ld"),
    (dict(max_steps=0), "max_steps")]
APPEND_REFUSALS = [(dict(**{k: None}), "null") for k in ("fin", "counts", "dstate", "istate", "ring", "head")] + [
    (dict(n=0), "65536"), (dict(n=65537), "65536"), (dict(capacity=7), "capacity"), (dict(n=600, capacity=599), "capacity"),
    (dict(half=2), "half"), (dict(half=-1), "half"), (dict(vstep=-1), "count up"), (dict(updates=-1), "count up")]


@pytest.mark.parametrize("over,fragment", STEP_REFUSALS, ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in STEP_REFUSALS])
def test_episode_step_refuses_before_launching(lib, over, fragment):
    kw, keep = step_args()
    assert fragment in refused(lib, "nlbac_episode_step", dict(kw, **over), str(over))


@pytest.mark.parametrize("over,fragment", APPEND_REFUSALS,
                         ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in APPEND_REFUSALS])
def test_episode_append_refuses_before_launching(lib, over, fragment):
    kw, keep = append_args()
    assert fragment in refused(lib, "nlbac_episode_append", dict(kw, **over), str(over))


@pytest.mark.parametrize("shift", [4, 8, 12])
def test_episode_append_refuses_a_misaligned_ring(lib, shift):
    kw, keep = append_args()
    assert "16 bytes" in refused(lib, "nlbac_episode_append", dict(kw, ring=kw["ring"] + shift), "ring + %d" % shift)


def test_the_entries_are_declared_under_abi_17(lib):
    from nlbac_amd import _lib
    assert _lib.ABI_VERSION == 17 == lib.nlbac_abi_version()
    assert {"nlbac_episode_step", "nlbac_episode_append"} <= set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "nlbac_hip.h")).read()
    assert re.search(r"int nlbac_episode_step\(", header) and re.search(r"int nlbac_episode_append\(", header)
