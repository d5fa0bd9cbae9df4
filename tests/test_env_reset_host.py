"""Host-side checks of the simulators' resets on the device (``envs/device.py`` ``device_resets=True``,
``csrc/env_reset_kernels.hip``): the numpy restatement of the SimulatedCars reset draw (``cars_reset_offset`` below — the
GPU tests import it), the two entry points' declarations and refusals (no GPU needed: every pointer handed over is host
memory that a refused call never touches), and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_rollout_concat_host import lib, refused      # noqa: F401  (lib: the fixture that builds and loads)

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: ``ctr`` four and ``key`` two uint32 arrays (or scalars) that
    broadcast; returns the four output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & M32 for w in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(w, dtype=np.uint64) & M32 for w in key)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [w.astype(np.uint32) for w in c]


def cars_reset_offset(seed, lane, count):
    """The N(0, 0.5) initial-velocity offset of lane ``lane``'s reset number ``count`` under ``seed`` (csrc/philox.h has
    the definition): float64, arrays broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x, y, z, w = (v.astype(np.uint64) for v in philox4x32_10((lane, count, 0, 2), (seed & 0xFFFFFFFF, seed >> 32)))
    m1 = (x << np.uint64(20)) | (y >> np.uint64(12))
    m2 = (z << np.uint64(20)) | (w >> np.uint64(12))
    u1 = (m1.astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (m2.astype(np.float64) + 0.5) * 2.0 ** -52
    return 0.5 * (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2))


def test_philox_known_answer():
    got = [int(v[0]) for v in philox4x32_10((0, 0, 0, 0), (0, 0))]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [hex(v) for v in got]
    # (the second vector of the Random123 known-answer file: all ones)
    got = [int(v[0]) for v in philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD], [hex(v) for v in got]


def test_uniforms_are_exact_and_inside_the_unit_interval():
    for m in (0, 1, 2 ** 52 - 1):
        u = (np.float64(m) + 0.5) * 2.0 ** -52
        assert 0.0 < u < 1.0 and u * 2.0 ** 52 - 0.5 == m


def test_draw_statistics():
    """65536 draws of N(0, 0.5): five standard errors of the mean (0.5 / sqrt(n)) and of the std (0.5 / sqrt(2 n))."""
    off = cars_reset_offset(0, np.arange(65536), 0)
    mean, std = float(off.mean()), float(off.std())
    print("mean %.5f std %.5f" % (mean, std))
    assert abs(mean) <= 0.01 and abs(std - 0.5) <= 0.007
    assert np.abs(off).max() < 3.0
    assert not np.array_equal(off, cars_reset_offset(3, np.arange(65536), 0))
    assert not np.array_equal(off, cars_reset_offset(0, np.arange(65536), 1))


NAMES = ("nlbac_env_reset_rows", "nlbac_cars_env_reset")


def test_entry_points_are_declared():
    from nlbac_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nlbac_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.ABI_VERSION == 17 and "#define NLBAC_ABI_VERSION 17" in header


def test_library_exports_them(lib):
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert lib.nlbac_abi_version() == 17


def reset_args(name):
    """The arguments of a call of ``name`` that would be launched, by name and in the entry point's order."""
    from nlbac_amd import _lib
    host = (C.c_double * 64)()                   # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    if name == "nlbac_env_reset_rows":
        kw = dict(n=4, done=p, state_dim=3, obs_dim=7, start_state=p, start_obs=p, start_last_dist=1.0, state=p,
                  ep_step=p, last_dist=p, obs=p, obs32=p, reset_count=p, s=None)
    else:
        kw = dict(n=4, done=p, seed=0, noise=p, state=p, t=p, ep_step=p, obs=p, obs32=p, reset_count=p, reset_noise=p,
                  s=None)
    assert len(kw) == len(_lib._PROTOS[name]), name
    return kw, host


@pytest.mark.parametrize("name", NAMES)
def test_refuses_before_launching(lib, name):
    kw, keep = reset_args(name)
    assert "n >= 1" in refused(lib, name, dict(kw, n=0), "n = 0")
    assert "n >= 1" in refused(lib, name, dict(kw, n=-3), "n < 0")
    required = [k for k in kw if k not in ("n", "done", "seed", "noise", "state_dim", "obs_dim", "start_last_dist",
                                           "last_dist", "s")]
    assert len(required) == 7
    for k in required:
        assert "null pointer" in refused(lib, name, dict(kw, **{k: None}), "a null %s" % k)
    if name == "nlbac_env_reset_rows":
        assert "state_dim" in refused(lib, name, dict(kw, state_dim=0), "state_dim = 0")
        assert "obs_dim" in refused(lib, name, dict(kw, obs_dim=65), "obs_dim = 65")


def test_command_line_parses():
    from nlbac_amd.train import get_args
    a = get_args(["--env", "SimulatedCars", "--vector_envs", "8"])
    assert a.env == "SimulatedCars" and a.vector_envs == 8 and a.vector_device_resets is False
    b = get_args(["--env", "Unicycle", "--vector_envs", "8", "--vector_device_resets"])
    assert b.vector_device_resets is True


def test_make_takes_device_resets():
    import inspect
    from nlbac_amd.envs import device as D
    assert inspect.signature(D.make).parameters["device_resets"].default is False
    for cls in (D.DeviceUnicycleEnv, D.DevicePvtolEnv, D.DeviceSimulatedCarsEnv):
        assert inspect.signature(cls.__init__).parameters["device_resets"].default is False
        assert callable(getattr(cls, "reset_done"))
