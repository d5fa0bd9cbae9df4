"""Which kernel family serves a net is a function of the net's shape alone (no GPU needed).

The host answers that Python caches for the life of an object — the layout of a net's parameter pack
(``nlbac_mlp_pack_layout``) and the ``*_ok`` / ``*_mask_words`` queries — are pinned for every shape class, and they
do not move when the process environment carries the names of the kernel switches ``csrc/`` once read with ``getenv``
("Retired since")."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_layers, in, hid, out) -> (masks_ok, fwd_head_ok, has 32x32x2 tile packs, packed_floats)
MLPS = {
    (3, 9, 256, 1): (1, 1, False, 143360), (3, 2, 256, 1): (1, 1, False, 143360), (3, 7, 256, 4): (1, 1, False, 143360),
    (3, 13, 128, 2): (1, 1, False, 38912),
    (3, 5, 64, 3): (1, 0, False, 11264),
    (3, 16, 256, 1): (0, 0, True, 278528), (3, 9, 256, 17): (0, 0, True, 278528),
    (3, 3, 100, 3): (0, 0, True, 27648),
    (3, 4, 96, 5): (0, 0, True, 19200),
    (3, 9, 192, 1): (0, 0, True, 159744),
    (4, 9, 256, 1): (0, 0, True, 266240),
    (2, 3, 8, 2): (0, 0, True, 256),
    (5, 3, 100, 3): (0, 0, True, 148480),
    (4, 12, 64, 10): (0, 0, True, 33792),
}

# (ns, nu, hid, f layers, g layers) -> (rk_interp_ok, node_adj_interp_ok, mask_words(0), mask_words(1))
AFFINE = {
    (3, 2, 100, 5, 4): (1, 1, 4, 4), (3, 2, 64, 5, 4): (1, 1, 4, 4), (3, 2, 128, 5, 4): (1, 1, 4, 4),
    (6, 2, 100, 5, 4): (1, 1, 4, 4), (4, 4, 64, 5, 4): (1, 1, 4, 4), (5, 2, 64, 5, 4): (1, 1, 4, 4),
    (3, 2, 160, 5, 4): (0, 0, 5, 5),
    (3, 2, 232, 5, 4): (0, 0, 8, 8),
    (3, 2, 100, 4, 4): (0, 0, 4, 4),
    (3, 2, 96, 5, 4): (0, 0, 3, 3),
    (5, 3, 64, 5, 4): (0, 0, 2, 2),
}

# (in, hid, out, n_layers) -> (rk_interp_ok with g = NULL, concat_adj_step_ok, concat_rk_mask_words)
SINGLE = {
    (12, 64, 10, 4): (1, 1, 4), (15, 64, 11, 4): (1, 1, 4), (12, 100, 10, 4): (1, 1, 4), (12, 128, 10, 4): (1, 1, 4),
    (12, 160, 10, 4): (0, 0, 0), (12, 64, 10, 5): (0, 0, 0), (20, 64, 16, 4): (0, 0, 0), (21, 64, 16, 4): (0, 0, 0),
    (12, 96, 10, 4): (0, 0, 0),
}

# the switches csrc/ once read: thirteen booleans ("0" = the older kernels) and a forced wave count
RETIRED = ["NLBAC_MLP_WAVES8", "NLBAC_MLP_DW64", "NLBAC_MLP_OCC", "NLBAC_MLP_RR", "NLBAC_MLP_RR_BWD", "NLBAC_MLP_RRQ",
           "NLBAC_MLP_DW16", "NLBAC_NODE_RR", "NLBAC_NODE_SPLIT", "NLBAC_CONCAT_RR", "NLBAC_ADJ_RR", "NLBAC_ADJ_RR_KEEP",
           "NLBAC_CONCAT_ADJ_RR"]
RETIRED_ENV = dict({name: "0" for name in RETIRED}, NLBAC_CONCAT_NW="2")


def answers():
    """The three tables as this process's library answers them: {"mlp" / "affine" / "single": [[key, values], ...]}."""
    import nlbac_amd  # noqa: F401
    from nlbac_amd import _lib
    C = _lib.C
    _lib.build()
    lib = _lib.load()

    def net(n_layers, in_dim, hid, out_dim):
        m = _lib.Mlp()
        m.n_layers, m.in_dim, m.hid, m.out_dim = n_layers, in_dim, hid, out_dim
        lib.nlbac_mlp_pack_layout(C.byref(m))
        return m

    out = {"mlp": [], "affine": [], "single": []}
    for key in MLPS:
        m = net(*key)
        tile_packs = [m.pf_off[l] >= 0 for l in range(m.n_layers - 1)]
        assert all(tile_packs) or not any(tile_packs), (key, tile_packs)
        out["mlp"].append([list(key), [lib.nlbac_mlp_masks_ok(C.byref(m), 1), lib.nlbac_mlp_fwd_head_ok(C.byref(m), 1),
                                       tile_packs[0], m.packed_floats]])
    for key in AFFINE:
        ns, nu, hid, f_layers, g_layers = key
        f, g = net(f_layers, ns, hid, ns), net(g_layers, ns, hid, ns * nu)
        out["affine"].append([list(key), [lib.nlbac_rk_interp_ok(C.byref(f), C.byref(g)),
                                          lib.nlbac_node_adj_interp_ok(C.byref(f), C.byref(g)),
                                          lib.nlbac_node_rk_mask_words(C.byref(f), C.byref(g), 0),
                                          lib.nlbac_node_rk_mask_words(C.byref(f), C.byref(g), 1)]])
    for key in SINGLE:
        in_dim, hid, out_dim, n_layers = key
        m = net(n_layers, in_dim, hid, out_dim)
        out["single"].append([list(key), [lib.nlbac_rk_interp_ok(C.byref(m), None), lib.nlbac_concat_adj_step_ok(C.byref(m)),
                                          lib.nlbac_concat_rk_mask_words(C.byref(m))]])
    return out


def check(got):
    """Every row of `got` (answers(), possibly through JSON) against the tables; all differing rows in the message."""
    wrong = []
    for name, table in (("mlp", MLPS), ("affine", AFFINE), ("single", SINGLE)):
        assert [tuple(k) for k, _ in got[name]] == list(table)
        wrong += [(name, tuple(k), tuple(v), table[tuple(k)]) for k, v in got[name] if tuple(v) != table[tuple(k)]]
    assert not wrong, "%d rows differ (table, shape, got, want): %s" % (len(wrong), wrong)


def test_kernel_pick_answers_per_shape_class():
    assert len(MLPS) + len(AFFINE) + len(SINGLE) == 34
    check(answers())


def test_kernel_pick_ignores_the_retired_environment_switches():
    assert len(RETIRED_ENV) == 14
    code = ("import sys; sys.path[:0] = [%r, %r]; import nlbac_amd, json, test_kernel_pick_host as T; "
            "print(json.dumps(T.answers()))" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **RETIRED_ENV), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    check(json.loads(r.stdout.strip().splitlines()[-1]))
