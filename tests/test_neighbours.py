"""Point neighbourhoods without a GPU: the host mirror hns_grid_point_neighbours (leafio.point_neighbours) against the numpy restatement of tests/neighbour_cases.py, bytes
of count, density and push; the conditions the point sets must meet, on the restatement's count; the symmetry and the reflection of the lattice set; the refusals of the C
ABI that need no device; the bindings. tests/test_neighbours_gpu.py holds the device's query to the same mirror."""
import ctypes as C
import os

import numpy as np
import pytest

import neighbour_cases as nc
import order_cases as oc
import sequence_cases as sq
from hnanosolver_amd import _lib, device, leafio
from hnanosolver_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.HNS_ERR_INVALID_ARGUMENT
F = np.float32
SYMBOLS = ("hns_point_order_cells", "hns_point_order_neighbours", "hns_grid_point_neighbours")
EIGHT = tuple(n for n in nc.GRIDS if nc.corner_of_eight(oc.origins(n)) is not None)  # the grids where eight leaves meet in a corner


def test_the_grids_hold_what_the_conditions_need():
    assert "dense32" in EIGHT and "one_leaf" not in EIGHT, EIGHT


@pytest.mark.parametrize("name", nc.GRIDS)
def test_point_sets_meet_their_conditions(name):
    """(a) .. (g) and (i) of the full set at h = 2, each with its minimum; (a) and (i) where eight leaves meet in a corner of the grid"""
    xyz = nc.full_set(name)
    assert xyz.shape == (nc.N_POINTS, 3) and xyz.dtype == F
    c = nc.conditions(name, 2.0)
    print(name, c)
    if name in EIGHT:
        assert c["face"] >= 100 and c["edge"] >= 50 and c["corner"] >= 10, (name, c)            # (a)
        assert c["leaves_of_one_points_neighbours"] == 8, (name, c)                            # (i)
    assert c["box_into_absent_leaf"] >= 100, (name, c)                                        # (b)
    assert c["outside_within_h"] >= 20 and c["outside_unrelated"], (name, c)                   # (c)
    assert c["coincident_pairs"] >= 40, (name, c)                                              # (d)
    assert c["integer"] >= 100 and c["on_leaf_face"] >= 10, (name, c)                          # (e)
    assert c["fullest_voxel"] > 256 and c["voxels_of_65"] >= 1, (name, c)                      # (f)
    assert c["nan_rows"] >= 4 and c["plus_inf_rows"] >= 2 and c["minus_inf_rows"] >= 2 and c["rows_at_2^23"] >= 3, (name, c)  # (g)
    if name in ("ragged32", "dense32"):  # (the grids that straddle a power of two, where x + h changes binade)
        assert c["six_cell_boxes"] >= 10, (name, c)  # x + h rounded up to an integer: the sixth cell of a box


@pytest.mark.parametrize("name", EIGHT)
def test_some_prefix_leaves_a_leaf_empty_between_populated_ones(name):
    """(h)"""
    found = {count: nc.empty_leaf_between_populated(name, count) for count in nc.COUNTS}
    print(name, found)
    assert max(found.values()) >= 1, (name, found)


@pytest.mark.parametrize("radius", nc.RADII)
@pytest.mark.parametrize("name", nc.GRIDS)
def test_host_mirror_matches_the_restatement(name, radius):
    g = oc.host_grid(name)
    for count in nc.COUNTS:
        xyz = nc.points(name, count)
        before = xyz.copy()
        got = leafio.point_neighbours(g, xyz, radius)
        assert got[0].dtype == np.uint32 and got[1].dtype == F and got[2].shape == (count, 3)
        nc.same(got, nc.expected(name, count, radius), f"{name} radius {radius} count {count}")
        assert xyz.tobytes() == before.tobytes()
    assert int(nc.expected(name, nc.N_POINTS, radius).count.sum()) >= 1000, "the full set has too few pairs to tell anything"


def test_outputs_may_be_left_out():
    g = oc.host_grid("ragged32")
    xyz = nc.points("ragged32", 257)
    want = nc.expected("ragged32", 257, 1.0)
    count, density, push = np.zeros(257, dtype=np.uint32), np.zeros(257, dtype=F), np.zeros((257, 3), dtype=F)
    for mask in range(1, 8):
        outs = [a if mask >> b & 1 else None for b, a in enumerate((count, density, push))]
        for a in (count, density, push):
            a.view(np.uint32)[...] = 0xDEADBEEF
        _lib.check(lib.hns_grid_point_neighbours(g.ptr, xyz.ctypes.data, 257, 1.0, *[None if a is None else a.ctypes.data for a in outs]))
        for b, (a, w) in enumerate(zip((count, density, push), want[:3])):
            if mask >> b & 1:
                assert a.tobytes() == w.tobytes(), (mask, b)
            else:
                assert (a.view(np.uint32) == 0xDEADBEEF).all(), (mask, b)


@pytest.mark.parametrize("radius", nc.LATTICE_RADII)
def test_lattice_set_symmetry_and_reflection(radius):
    """on multiples of 2^-8 the pair relation is symmetric and a reflection through the box centre keeps count and density and negates the push in every bit: asserted
    on the restatement, then on the host mirror"""
    name = nc.LATTICE_GRID
    o = oc.origins(name)
    assert set(map(tuple, (24 - o).tolist())) == set(map(tuple, o.tolist())), "the grid's leaves do not reflect onto themselves"
    assert float(F(radius)) * 256.0 == round(radius * 256.0)
    g, L = oc.host_grid(name), len(o)
    x = nc.lattice_set()
    r = nc.restate(g, L, x, radius)
    m = nc.restate(g, L, nc.reflected(x), radius)
    assert int(r.count.sum()) >= 2000 and int(r.count.sum()) % 2 == 0
    pairs = set(map(tuple, r.pairs.tolist()))
    assert all((j, i) in pairs for i, j in pairs), "the pair relation is not symmetric"
    assert int((r.d2 == 0).sum()) >= 40
    nc.same((m.count, m.density, m.push), (r.count, r.density, nc.negated_push(r.push)), f"the restatement under reflection, radius {radius}")
    assert np.count_nonzero(r.push) >= 1000
    nc.same(leafio.point_neighbours(g, x, radius), r, f"the mirror on the lattice set, radius {radius}")
    nc.same(leafio.point_neighbours(g, nc.reflected(x), radius), (r.count, r.density, nc.negated_push(r.push)), f"the mirror under reflection, radius {radius}")


@pytest.mark.parametrize("name", ["ragged32", "sparse_far"])
def test_a_shuffle_of_the_input_permutes_the_outputs(name):
    g = oc.host_grid(name)
    xyz = nc.full_set(name)
    p = np.random.default_rng(8).permutation(len(xyz))
    for radius in (0.73, 2.0):
        a = leafio.point_neighbours(g, xyz, radius)
        b = leafio.point_neighbours(g, np.ascontiguousarray(xyz[p]), radius)
        nc.same(b, tuple(v[p] for v in a), f"{name} radius {radius}: shuffled")


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_host_mirror_refusals_touch_nothing():
    who = "hns_grid_point_neighbours"
    g = oc.host_grid("ragged32")
    xyz = np.array(nc.points("ragged32", 64))
    before = xyz.copy()
    count, density, push = np.full(64, 0xDEADBEEF, dtype=np.uint32), np.full(64, 7.0, dtype=F), np.full((64, 3), 7.0, dtype=F)
    x, c, d, p = xyz.ctypes.data, count.ctypes.data, density.ctypes.data, push.ctypes.data
    _refused(lib.hns_grid_point_neighbours(None, x, 64, 1.0, c, d, p), who, "grid")
    _refused(lib.hns_grid_point_neighbours(g.ptr, None, 64, 1.0, c, d, p), who, "xyz")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 2 ** 31, 1.0, c, d, p), who, "n is above")
    for bad in (0.0, -1.0, float("nan"), 2.0000002, float("inf")):
        _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, bad, c, d, p), who, "radius")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, 1.0, None, None, None), who, "all null")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, 1.0, c, x, p), who, "xyz")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, 1.0, c, d, x), who, "xyz")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, 1.0, c, p, p), who, "same buffer")
    _refused(lib.hns_grid_point_neighbours(g.ptr, x, 64, 1.0, p, d, p), who, "same buffer")
    assert (count == 0xDEADBEEF).all() and (density == 7.0).all() and (push == 7.0).all() and xyz.tobytes() == before.tobytes()
    assert lib.hns_grid_point_neighbours(g.ptr, None, 0, 1.0, None, None, p) == _lib.HNS_OK and (push == 7.0).all()  # n == 0: nothing is looked at
    assert lib.hns_grid_point_neighbours(g.ptr, x, 64, 2.0, c, d, p) == _lib.HNS_OK  # (the largest radius is taken)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        leafio.point_neighbours(g, xyz.reshape(-1), 1.0)


def test_object_refusals_that_need_no_device():
    table = C.c_void_p(0)
    _refused(lib.hns_point_order_cells(None, C.byref(table)), "hns_point_order_cells", "null point order")
    _refused(lib.hns_point_order_neighbours(None, None, 0, 1.0, None, None, None), "hns_point_order_neighbours", "null point order")
    assert table.value is None


def test_the_symbols_are_bound_exported_and_operations_of_the_sequences():
    header = open(os.path.join(ROOT, "include", "hns.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and callable(getattr(lib, name)) and f" {name}(" in header, name
    assert lib.hns_version() == 100
    for name in SYMBOLS[:2]:  # the object's calls: operations of the call-sequence vocabulary that some committed script holds, and no exemption
        ops = [k for k, o in sq.OPS.items() if name in o.symbols]
        assert ops and name not in sq.EXEMPT, name
        assert [s.name for s in sq.SCRIPTS if set(ops) & {k for k, _ in s.steps}], f"no committed script holds an operation of {name}"
    assert hasattr(device.PointOrder, "neighbours") and isinstance(device.PointOrder.cell_start, property) and callable(leafio.point_neighbours)


@pytest.mark.parametrize("name", nc.GRIDS)
def test_cell_table_of_the_mirrors_keys_is_searchsorted(name):
    """what the device's table is held to: the restatement's cell_table of leafio.sort_points' keys, against a count by voxel of the points that take part"""
    g, L = oc.host_grid(name), len(oc.origins(name))
    xyz = nc.full_set(name)
    _, keys, leaf_start = leafio.sort_points(g, xyz, "voxel")
    table = nc.cell_table(keys, L)
    assert len(table) == 512 * L + 1 and int(table[0]) == 0 and int(table[-1]) == int(leaf_start[L])
    assert np.array_equal(table, np.searchsorted(keys[: leaf_start[L]], np.arange(512 * L + 1)).astype(np.uint32))
    part = nc.takes_part(g, L, xyz)
    per_voxel = np.bincount(oc.voxel_keys(g, L, xyz)[part].astype(np.int64), minlength=512 * L)
    assert np.array_equal(np.diff(table.astype(np.int64)), per_voxel)
    assert np.array_equal(table[::512][: L + 1], leaf_start[: L + 1])  # (a leaf's first voxel starts the leaf)
