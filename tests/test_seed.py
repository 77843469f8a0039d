"""The seeds of a point set without a GPU: hns_point_leaves (the host mirror of hns_dev_point_leaves) against the numpy restatement of include/hns.h in
tests/seed_cases.py, byte for byte, on every point set the GPU test uses; known answers; the query idiom and every refusal; the three new symbols exported, declared and
bound; and the condition the regrid tests rest on -- counted by the oracle --, that the point sets really reach outside their grids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import points_cases as pc
import seed_cases as sd
from hnanosolver_amd import _lib, device, leafio
from oracle_lib import OracleGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"hns_point_leaves": "int", "hns_dev_point_leaves": "int", "hns_sim_regrid_seeded": r"hns_grid\s*\*"}
F = np.float32


def header():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    decl = re.search(r"^%s\s*%s\s*\(([^;]*)\);" % (SYMBOLS[name], name), header(), re.M | re.S)
    assert decl, f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[name][0] is (C.c_int if SYMBOLS[name] == "int" else C.c_void_p)
    assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, "one ctypes argument per parameter of the declaration"


def test_python_mirrors_exist():
    assert callable(leafio.point_leaves) and callable(device.point_leaves) and callable(device.Sim.emit)
    assert device.Sim.last_seeds_skipped == 0
    assert "points" in device.Sim.regrid.__code__.co_varnames


def test_header_states_the_definition_once_and_keeps_the_splats_words():
    h = header()
    comment = h[: h.index("int hns_point_leaves")].rsplit("/*", 1)[1]
    assert "-8388608.0f <= c && c < 8388607.0f" in comment and "ALL EIGHT" in comment
    assert h.count("-8388608.0f") == 1, "the seed definition is stated once"
    splat = h[: h.index("int hns_sim_splat_points")].rsplit("/*", 1)[1]
    assert "CANNOT ADD LEAVES" in splat and "hns_sim_regrid_seeded" in splat
    seeded = h[: h.index("hns_grid* hns_sim_regrid_seeded")].rsplit("/*", 1)[1]
    assert "mirrored in hns_dist_*" in seeded


@pytest.mark.parametrize("name,count", sd.all_point_sets(), ids=lambda v: str(v))
def test_host_mirror_equals_the_restatement(name, count):
    xyz = sd.point_set(name, count)
    want, got = sd.seeds(xyz), leafio.point_leaves(xyz)
    assert sd.same(got, want), f"{name}[:{count}]: {len(got[0])} leaves against {len(want[0])}, skipped {got[2]} against {want[2]}"
    if len(xyz) > 1:  # the set of points decides, not their order or multiplicity
        rng = np.random.default_rng(5)
        again = np.concatenate([xyz[rng.permutation(len(xyz))], xyz[: len(xyz) // 3]])
        o, m, skipped = leafio.point_leaves(again)
        assert sd.same((o, m, 0), (want[0], want[1], 0)), f"{name}[:{count}]: permuted and repeated"


def test_known_answers():
    o, m, skipped = leafio.point_leaves(np.array([[3.25, 3.25, 3.25]], dtype=F))
    assert o.tolist() == [[0, 0, 0]] and skipped == 0
    want = np.zeros(64, dtype=np.uint8)
    want[[27, 28, 35, 36]] = 0x18
    assert np.array_equal(m[0], want)
    o, m, _ = leafio.point_leaves(np.array([[7.5, 7.5, 7.5]], dtype=F))
    assert sorted(map(tuple, o.tolist())) == sorted((x, y, z) for x in (0, 8) for y in (0, 8) for z in (0, 8))
    assert all(int(np.unpackbits(row).sum()) == 1 for row in m)
    o, m, _ = leafio.point_leaves(np.array([[-0.5, 0, 0]], dtype=F))
    assert sorted(map(tuple, o.tolist())) == [(-8, 0, 0), (0, 0, 0)]
    o, m, _ = leafio.point_leaves(np.array([[2.0, 3.0, 4.0]], dtype=F))  # an integer position: weights of 0 on seven taps, eight seeds all the same
    assert o.tolist() == [[0, 0, 0]] and int(np.unpackbits(m).sum()) == 8
    o, m, skipped = leafio.point_leaves(np.zeros((0, 3), dtype=F))
    assert o.shape == (0, 3) and m.shape == (0, 64) and skipped == 0


def test_skipped_on_the_edges_set():
    xyz = sd.point_set("edges")
    want = sd.seeds(xyz)
    assert 0 < want[2] < len(xyz), "the set holds points that seed and points that do not"
    assert leafio.point_leaves(xyz)[2] == want[2]
    # the last seeding cell: its upper taps are the last voxels a 21-bit leaf coordinate reaches
    o, m, skipped = leafio.point_leaves(np.array([[8388606.5, -8388608.0, 0.0]], dtype=F))
    assert skipped == 0 and o[:, 0].max() == 8388600 and o[:, 1].min() == -8388608


def test_the_query_idiom():
    lib = _lib.load_library()
    xyz = sd.point_set("ball")
    want = sd.seeds(xyz)
    n, skipped = C.c_uint64(99), C.c_uint64(99)
    assert lib.hns_point_leaves(xyz.ctypes.data, len(xyz), None, None, 0, C.byref(n), C.byref(skipped)) == 0
    assert n.value == len(want[0]) == 8 and skipped.value == 0  # set, not added to
    o = np.full((8, 3), 77, dtype=np.int32)
    m = np.full((8, 64), 77, dtype=np.uint8)
    n.value = 99
    assert lib.hns_point_leaves(xyz.ctypes.data, len(xyz), o.ctypes.data, m.ctypes.data, 7, C.byref(n), None) == 0  # cap too small: nothing written
    assert n.value == 8 and (o == 77).all() and (m == 77).all()
    assert lib.hns_point_leaves(xyz.ctypes.data, len(xyz), o.ctypes.data, None, 8, C.byref(n), None) == 0  # masks_out may be NULL
    assert np.array_equal(o, want[0]) and (m == 77).all()
    assert lib.hns_point_leaves(xyz.ctypes.data, len(xyz), o.ctypes.data, m.ctypes.data, 8, C.byref(n), C.byref(skipped)) == 0
    assert np.array_equal(m, want[1])


def test_refusals():
    lib = _lib.load_library()
    xyz = np.ones((2, 3), dtype=F)
    n = C.c_uint64(5)
    cases = [
        ((None, 2, None, None, 0, C.byref(n), None), "xyz is null"),
        ((xyz.ctypes.data, 2, None, None, 0, None, None), "n_leaves is null"),
        ((xyz.ctypes.data, 2 ** 31, None, None, 0, C.byref(n), None), "n is above 2^31 - 1"),
    ]
    for args, msg in cases:
        assert lib.hns_point_leaves(*args) == _lib.HNS_ERR_INVALID_ARGUMENT
        text = lib.hns_last_error().decode()
        assert text.startswith("hns_point_leaves:") and msg in text, text
    assert lib.hns_point_leaves(None, 0, None, None, 0, C.byref(n), None) == 0 and n.value == 0  # no point, no pointer looked at


def test_the_device_form_fails_loudly_without_a_device():
    lib = _lib.load_library()
    if lib.hns_device_count() > 0:
        pytest.skip("a HIP device is present; this test is for the CPU-only container")
    xyz = np.ones((2, 3), dtype=F)
    n = C.c_uint64(5)
    o = np.full((8, 3), 77, dtype=np.int32)
    assert lib.hns_dev_point_leaves(0, xyz.ctypes.data, 2, o.ctypes.data, None, 8, C.byref(n), None, None) == _lib.HNS_ERR_NO_DEVICE
    text = lib.hns_last_error().decode()
    assert "hns_dev_point_leaves" in text and "no CPU fallback" in text
    assert (o == 77).all()
    assert lib.hns_dev_point_leaves(0, xyz.ctypes.data, 2, None, None, 0, None, None, None) == _lib.HNS_ERR_INVALID_ARGUMENT  # its arguments are checked as the mirror's are


@pytest.mark.parametrize("name", [g for g in pc.GRIDS if g != "one_leaf"])
def test_the_point_sets_reach_outside_their_grids(name):
    """the condition every regrid test of tests/test_seed_gpu.py rests on, counted by the oracle: the domain really has to grow"""
    o, _, _, xyz = pc.case(name)
    G = OracleGrid(o)
    pc.check_conditions(G, xyz, name)
    share = sd.share_with_a_tap_outside(G, xyz)
    print(f"{name}: {share:.3f} of the points have a tap outside the domain")
    assert share >= 0.15
    have = set(map(tuple, np.asarray(o).tolist()))
    assert any(tuple(q) not in have for q in sd.seeds(xyz)[0].tolist()), "the seeds bring leaves the grid lacks"
