"""CPU: trajectory windows out of the replay (``ReplayMemory.sample_windows``, the argument checks of both replays) against
the validity rule written out push by push, the new entry points' declarations and bindings, and the agent options."""
import os
import random
import re
import types

import numpy as np
import pytest

import nlbac_amd  # noqa: F401
from fit_windows_common import CASES, episode_obs, ref_windows
from nlbac_amd import _lib
from nlbac_amd.sac_cbf_clf.replay_memory import DeviceReplayMemory, ReplayMemory, check_windows, window_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlbac_gather_windows", "nlbac_sample_windows", "nlbac_traj_mse_fwd_bwd")
OBS = 7


def filled(cap, lengths, lanes=1, cls=ReplayMemory):
    """A host replay holding the episodes; column ``reward`` carries the push number."""
    obs, nobs = episode_obs(lengths, OBS, lanes)
    mem = cls(cap, 0)
    for p in range(len(obs)):
        mem.push(obs[p], np.zeros(2), float(p), 0.0, np.zeros(2), np.zeros(2), nobs[p], 1.0, t=0.0, next_t=0.0)
    return mem, obs, nobs


@pytest.mark.parametrize("kw", [dict(batch_size=0), dict(horizon=0), dict(stride=0), dict(batch_size=-3), dict(horizon=True)])
def test_sizes_below_one_are_refused(kw):
    mem, _, _ = filled(64, (7, 5))
    args = dict(batch_size=4, horizon=2, stride=1)
    args.update(kw)
    with pytest.raises(ValueError):
        mem.sample_windows(**args)
    with pytest.raises(ValueError):
        check_windows(args["batch_size"], args["horizon"], args["stride"], 12, host_draw=False)


def test_more_starts_than_rows_and_windows_longer_than_the_replay_are_refused():
    mem, _, _ = filled(64, (7, 5))
    with pytest.raises(ValueError):
        mem.sample_windows(13, 2)                      # 12 rows, drawn without replacement
    mem.sample_windows(12, 2)
    with pytest.raises(ValueError):
        mem.sample_windows(4, 13)                      # (13 - 1) * 1 >= 12
    with pytest.raises(ValueError):
        mem.sample_windows(4, 3, stride=6)             # (3 - 1) * 6 >= 12
    mem.sample_windows(4, 12)
    check_windows(13, 2, 1, 12, host_draw=False)       # drawn on the device with replacement: any batch size
    with pytest.raises(ValueError):
        check_windows(4, 13, 1, 12, host_draw=False)


def test_device_replay_checks_before_it_touches_a_device():
    """The device replay's ``sample_windows`` refuses bad arguments before its first device call: an object with
    nothing but a length gets as far as the check."""
    stub = types.SimpleNamespace(_len=12, device_rng=False)
    for kw in (dict(batch_size=0, horizon=2), dict(batch_size=4, horizon=0), dict(batch_size=4, horizon=2, stride=0),
               dict(batch_size=13, horizon=2), dict(batch_size=4, horizon=13), dict(batch_size=4, horizon=3, stride=6)):
        with pytest.raises(ValueError):
            DeviceReplayMemory.sample_windows(stub, **kw)


@pytest.mark.parametrize("case", ["open", "full"])
def test_every_start_row_against_the_rule(case):
    cap, lengths, n_valid = CASES[case]
    mem, obs, nobs = filled(cap, lengths)
    P = len(obs)
    assert len(mem) == min(P, cap) and mem.position == P % cap
    starts = np.arange(len(mem))
    H = 3
    rows, valid = window_rows(starts, H, 1, len(mem), mem.capacity, mem.position, mem._cols[0], mem._cols[6])
    pushes, ref_valid = ref_windows(obs, nobs, cap, starts, H, 1)
    np.testing.assert_array_equal(valid, ref_valid)
    assert int(valid.sum()) == n_valid
    np.testing.assert_array_equal(mem._cols[2][rows], pushes.astype(np.float64))      # the reward column: the push number
    # through the public call: a permutation of all start rows
    random.seed(3)
    fields, v = mem.sample_windows(len(mem), H)
    assert len(fields) == 10 and v.shape == (len(mem),) and int(v.sum()) == n_valid
    assert fields[0].shape == (H, len(mem), OBS) and fields[2].shape == (H, len(mem))
    start_push = fields[2][0].astype(np.int64)
    assert sorted(start_push % cap) == list(range(len(mem)))
    p2, rv = ref_windows(obs, nobs, cap, start_push % cap, H, 1)
    np.testing.assert_array_equal(v, rv)
    np.testing.assert_array_equal(fields[2], p2.astype(np.float64))
    np.testing.assert_array_equal(fields[0], obs[p2].astype(np.float64))
    np.testing.assert_array_equal(fields[6], nobs[p2].astype(np.float64))
    for k in range(H - 1):                              # a valid window is a chain
        np.testing.assert_array_equal(fields[6][k][v], fields[0][k + 1][v])


def test_horizon_one_is_always_valid():
    mem, _, _ = filled(40, CASES["full"][1])
    fields, v = mem.sample_windows(40, 1)
    assert v.all() and fields[0].shape == (1, 40, OBS)


def test_two_interleaved_lanes_need_stride_two():
    lengths = (7, 5, 9, 4)
    mem, obs, nobs = filled(64, lengths, lanes=2)
    n = len(mem)
    assert n == 50
    starts = np.arange(n)
    for stride in (1, 2):
        rows, valid = window_rows(starts, 3, stride, n, mem.capacity, mem.position, mem._cols[0], mem._cols[6])
        pushes, ref_valid = ref_windows(obs, nobs, 64, starts, 3, stride)
        np.testing.assert_array_equal(valid, ref_valid)
        np.testing.assert_array_equal(mem._cols[2][rows], pushes.astype(np.float64))
        if stride == 1:
            assert not valid.any()                      # neighbouring rows belong to different lanes
        else:
            assert 0 < int(valid.sum()) < n             # a strict, non-empty subset
            assert int(valid.sum()) == 2 * sum(l - 2 for l in lengths)


def test_barrier_replay_finds_its_next_state_column():
    from nlbac_amd.neural_barrier_certificate.sac_cbf_clf.replay_memory import ReplayMemory as BarrierReplay
    obs, nobs = episode_obs((4, 3), OBS)
    mem = BarrierReplay(16, 0)
    for p in range(len(obs)):
        mem.push(obs[p], np.zeros(2), float(p), 0.0, -1.0, np.zeros(2), np.zeros(2), nobs[p], 1.0)
    random.seed(1)
    fields, v = mem.sample_windows(7, 2)
    assert len(fields) == 11
    _, rv = ref_windows(obs, nobs, 16, fields[2][0].astype(np.int64), 2, 1)
    np.testing.assert_array_equal(v, rv)
    assert int(v.sum()) == 3 + 2


def test_header_declares_and_binding_types_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "nlbac_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "%s is not declared in nlbac_hip.h" % name
        assert name in _lib.EXPORTS
    assert len(_lib._PROTOS["nlbac_gather_windows"]) == 16
    assert len(_lib._PROTOS["nlbac_sample_windows"]) == 17
    assert len(_lib._PROTOS["nlbac_traj_mse_fwd_bwd"]) == 11
    assert int(re.search(r"#define NLBAC_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 17


def test_library_exports_the_new_entry_points():
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.nlbac_abi_version() == 17


def test_node_horizon_defaults_to_one():
    from nlbac_amd.node_fit import node_fit_options
    from nlbac_amd.train import get_args
    from oracle.nlbac_oracle import Args
    assert node_fit_options(Args()) == (1, 1)
    assert node_fit_options(types.SimpleNamespace(node_horizon=3, node_stride=8)) == (3, 8)
    for bad in (dict(node_horizon=0), dict(node_stride=0), dict(node_horizon=-2)):
        with pytest.raises(ValueError):
            node_fit_options(types.SimpleNamespace(**bad))
    assert get_args([]).node_horizon == 1
    assert get_args(["--node_horizon", "3"]).node_horizon == 3


def test_train_rollout_step_sits_beside_train_step():
    from nlbac_amd import node_fit
    from nlbac_amd.sac_cbf_clf import model
    assert model.train_rollout_step is node_fit.train_rollout_step and callable(model.train_step)
