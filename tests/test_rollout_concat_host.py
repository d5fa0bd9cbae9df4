"""Host-side checks of the one-launch rollout and time-grid entry points of both NODE forms: where
``nlbac_concat_rk_traj_ok`` says yes, and that ``nlbac_{concat,node}_rk_{traj,grid}_{fwd,bwd}`` refuse bad arguments
with a message before anything is launched (no GPU needed: every pointer handed over here is host memory that a refused
call never touches)."""
import ctypes as C

import pytest

from nlbac_amd import _lib

FWD = ("nlbac_concat_rk_traj_fwd", "nlbac_concat_rk_grid_fwd", "nlbac_node_rk_traj_fwd", "nlbac_node_rk_grid_fwd")
BWD = ("nlbac_concat_rk_traj_bwd", "nlbac_concat_rk_grid_bwd", "nlbac_node_rk_traj_bwd", "nlbac_node_rk_grid_bwd")


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


def args(lib, name):
    """The arguments of a call of ``name`` that would be launched, by name and in the entry point's order."""
    affine, grid, fwd = "_node_" in name, "_grid_" in name, name.endswith("_fwd")
    host = (C.c_float * 64)()                    # stands in for every device buffer: never read by a refused call
    p = C.addressof(host)
    tab = dict(n=8, H=2, S=1, beta=_lib.fptr(0.0), c_out=_lib.fptr(1.0))
    tab.update(dict(hs=p, hs_host=_lib.fptr(0.02, 0.03)) if grid else dict(h=0.02))
    if affine:
        nets = (desc(lib, 5, 3, 64, 3), desc(lib, 4, 3, 64, 6))
        assert lib.nlbac_node_rk_traj_ok(C.byref(nets[0]), C.byref(nets[1])) == 1
        head = dict(f=C.byref(nets[0]), g=C.byref(nets[1]))
        if fwd:
            kw = dict(head, x0=p, u=p, **tab, out=p, K=p, Y=p, G=p, acts_f=None, ls_f=0, acts_g=None, ls_g=0, bits=0, s=None)
        else:
            kw = dict(head, u=p, **tab, G=p, acts_f=p, ls_f=8 * 2 * 4, acts_g=p, ls_g=8 * 2 * 4, bits=1, dout=p, dx0=p,
                      du=p, dK=None, dG=None, dz_f=None, dz_g=None, s=None)
    else:
        nets = (desc(lib, 4, 12, 100, 10),)
        head = dict(net=C.byref(nets[0]))
        if fwd:
            kw = dict(head, x0=p, c=p, **tab, out=p, Xin=None, acts=None, ls=0, bits=0, norm=None, s=None)
        else:
            kw = dict(head, **tab, acts=p, ls=8 * 2 * 4, bits=1, norm=None, dout=p, dx0=p, dc=p, dK=None, dz=None, s=None)
    return kw, (nets, host)


def refused(lib, name, kw, what):
    rc = getattr(lib, name)(*kw.values())
    assert rc == -1, "%s accepted %s" % (name, what)
    msg = lib.nlbac_last_error().decode()
    assert name in msg, (what, msg)
    return msg


def refuses_bad_steps(lib, name, kw):
    if "_grid_" in name:
        assert "positive" in refused(lib, name, dict(kw, hs_host=_lib.fptr(0.02, 0.0)), "a step of 0")
        assert "null" in refused(lib, name, dict(kw, hs_host=None), "a null hs_host")
    else:
        assert "positive" in refused(lib, name, dict(kw, h=0.0), "h = 0")
        assert "positive" in refused(lib, name, dict(kw, h=-0.02), "h < 0")


@pytest.mark.parametrize("name", FWD)
def test_forward_refuses_before_launching(lib, name):
    kw, keep = args(lib, name)
    assert "intervals" in refused(lib, name, dict(kw, H=0), "H = 0")
    refuses_bad_steps(lib, name, kw)
    assert "null" in refused(lib, name, dict(kw, out=None), "a null out")
    bad_bits = 3 if "_node_" in name else 2
    assert "acts_bits" in refused(lib, name, dict(kw, bits=bad_bits), "acts_bits = %d" % bad_bits)
    assert "intervals" in refused(lib, name, dict(kw, n=1 << 20, H=1 << 11), "H S n >= 2^31")


@pytest.mark.parametrize("name", BWD)
def test_backward_refuses_before_launching(lib, name):
    kw, keep = args(lib, name)
    p = kw["dout"]
    assert "intervals" in refused(lib, name, dict(kw, H=0), "H = 0")
    refuses_bad_steps(lib, name, kw)
    assert "null" in refused(lib, name, dict(kw, dx0=None), "a null dx0")
    if "_node_" in name:
        assert "acts_bits" in refused(lib, name, dict(kw, bits=3), "acts_bits = 3")
        assert "bit masks" in refused(lib, name, dict(kw, bits=1, dK=p, dG=p, dz_f=p, dz_g=p), "acts_bits = 1 with dz")
        assert "together" in refused(lib, name, dict(kw, bits=0, dz_f=p), "dz_f without dz_g, dG and dK")
    else:
        assert "acts_bits" in refused(lib, name, dict(kw, bits=2), "acts_bits = 2")
        assert "mask words" in refused(lib, name, dict(kw, bits=1, dK=p, dz=p), "acts_bits = 1 with dz")
        assert "together" in refused(lib, name, dict(kw, bits=0, dz=p), "dz without dK")
    assert "intervals" in refused(lib, name, dict(kw, n=1 << 20, H=1 << 11), "H S n >= 2^31")
