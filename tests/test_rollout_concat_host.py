"""Host-side checks of the single-net NODE's one-launch rollout entry points: where ``nlbac_concat_rk_traj_ok`` says
yes, and that ``nlbac_concat_rk_traj_fwd`` / ``_bwd`` refuse bad arguments with a message before anything is launched
(no GPU needed: every pointer handed over here is host memory that a refused call never touches)."""
import ctypes as C

import pytest

from nlbac_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def desc(lib, layers, in_dim, hid, out_dim):
    net = _lib.Mlp()
    net.n_layers, net.in_dim, net.hid, net.out_dim = layers, in_dim, hid, out_dim
    assert lib.nlbac_mlp_pack_layout(C.byref(net)) > 0
    return net


def test_traj_ok_follows_the_register_resident_kernels(lib):
    for hid in (100, 64, 128):
        assert lib.nlbac_concat_rk_traj_ok(C.byref(desc(lib, 4, 12, hid, 10))) == 1, hid
    assert lib.nlbac_concat_rk_traj_ok(C.byref(desc(lib, 4, 15, 64, 11))) == 1       # the widest input: 15 + the bias column
    assert lib.nlbac_concat_rk_traj_ok(C.byref(desc(lib, 4, 12, 256, 10))) == 0
    assert lib.nlbac_concat_rk_traj_ok(C.byref(desc(lib, 4, 16, 64, 12))) == 0
    assert lib.nlbac_concat_rk_traj_ok(C.byref(desc(lib, 3, 12, 64, 10))) == 0
    assert lib.nlbac_concat_rk_traj_ok(None) == 0


def args(lib):
    net = desc(lib, 4, 12, 100, 10)
    host = (C.c_float * 64)()                    # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    beta, c_out = _lib.fptr(0.0), _lib.fptr(1.0)
    fwd = dict(net=C.byref(net), x0=p, c=p, n=8, H=2, S=1, beta=beta, c_out=c_out, h=0.02, out=p, Xin=None, acts=None,
               ls=0, bits=0, norm=None, s=None)
    bwd = dict(net=C.byref(net), n=8, H=2, S=1, beta=beta, c_out=c_out, h=0.02, acts=p, ls=8 * 2 * 4, bits=1, norm=None,
               dout=p, dx0=p, dc=p, dK=None, dz=None, s=None)
    return fwd, bwd, (net, host)


def refused(lib, name, kw, what):
    rc = getattr(lib, name)(*kw.values())
    assert rc == -1, "%s accepted %s" % (name, what)
    msg = lib.nlbac_last_error().decode()
    assert name in msg, (what, msg)
    return msg


def test_forward_refuses_before_launching(lib):
    fwd, _, keep = args(lib)
    assert "intervals" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, H=0), "H = 0")
    assert "positive" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, h=0.0), "h = 0")
    assert "positive" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, h=-0.02), "h < 0")
    assert "null" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, out=None), "a null out")
    assert "acts_bits" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, bits=2), "acts_bits = 2")
    assert "intervals" in refused(lib, "nlbac_concat_rk_traj_fwd", dict(fwd, n=1 << 20, H=1 << 11), "H S n >= 2^31")


def test_backward_refuses_before_launching(lib):
    _, bwd, keep = args(lib)
    p = bwd["dout"]
    assert "intervals" in refused(lib, "nlbac_concat_rk_traj_bwd", dict(bwd, H=0), "H = 0")
    assert "positive" in refused(lib, "nlbac_concat_rk_traj_bwd", dict(bwd, h=0.0), "h = 0")
    assert "null" in refused(lib, "nlbac_concat_rk_traj_bwd", dict(bwd, dx0=None), "a null dx0")
    assert "mask words" in refused(lib, "nlbac_concat_rk_traj_bwd", dict(bwd, bits=1, dK=p, dz=p), "acts_bits = 1 with dz")
    assert "together" in refused(lib, "nlbac_concat_rk_traj_bwd", dict(bwd, bits=0, dz=p), "dz without dK")
