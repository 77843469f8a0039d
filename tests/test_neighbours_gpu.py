"""Point neighbourhoods on the GPU: device.PointOrder.cell_start and .neighbours (hns_point_order_cells, hns_point_order_neighbours: the kernels of hns_neighbours.hip)
against the host mirror leafio.point_neighbours, which tests/test_neighbours.py holds to the numpy restatement. Every comparison is equality of bytes: the sums are
integers, so the result is unique. Grids, point sets and their conditions are tests/neighbour_cases.py's."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import neighbour_cases as nc
import order_cases as oc
import pool_cases
import stream_cases as sc
from hnanosolver_amd import _lib, api, device, leafio
from hnanosolver_amd._lib import lib

pytestmark = pytest.mark.gpu

F = np.float32
BAD = _lib.HNS_ERR_INVALID_ARGUMENT
EXTRA = 5  # guard rows behind every output
ROWS = ("original", "ranked")


def torch():
    import torch as t

    return t


@functools.lru_cache(maxsize=None)
def dev_grid(name):
    return api.create_grid_from_leaves(oc.origins(name), oc.VS)


def to_dev(a):
    return torch().from_numpy(np.array(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32).copy()


@functools.lru_cache(maxsize=None)
def mirror(name, count, radius):
    """the host mirror on a prefix of the grid's set: computed once, shared, never written"""
    got = leafio.point_neighbours(oc.host_grid(name), nc.points(name, count), radius)
    for a in got:
        a.setflags(write=False)
    return got


def table_of(name, xyz):
    return nc.cell_table(leafio.sort_points(oc.host_grid(name), xyz, "voxel")[1], len(oc.origins(name)))


def outputs(n):
    """count, density and push of n rows and EXTRA guard rows each, inside guard bands, holding the sentinel"""
    slab = sc.Slab(torch(), {"count": ((n + EXTRA,), np.int32), "density": ((n + EXTRA,), F), "push": ((n + EXTRA, 3), F)}, device="cuda")
    for v in slab.views.values():
        sc.sentinel(v)
    return slab


def check_outputs(slab, n, asked, want, what):
    """the outputs asked for hold `want` in their n rows; everything else -- the rows behind, the outputs not asked for, the guard bands -- is untouched"""
    slab.check(what)
    for k, name in enumerate(("count", "density", "push")):
        got = u32(slab.views[name]).reshape(n + EXTRA, -1)
        assert (got[n:] == sc.OUT_WORD).all(), f"{what}: rows of {name} behind n were written"
        if name in asked and n:
            w = np.ascontiguousarray(want[k]).view(np.uint32).reshape(n, -1)
            bad = np.flatnonzero((got[:n] != w).any(1))
            assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} of {n} rows, first at {bad[:4].tolist()}: {got[bad[:4]].tolist()} against {w[bad[:4]].tolist()}"
        else:
            assert (got[:n] == sc.OUT_WORD).all(), f"{what}: {name} was not asked for and was written"


@pytest.mark.parametrize("name", nc.GRIDS)
def test_cell_table_is_searchsorted_of_the_mirrors_keys(name):
    grid = dev_grid(name)
    po = device.PointOrder(grid, nc.N_POINTS)
    for count in nc.COUNTS:
        xyz = nc.points(name, count)
        po.sort(to_dev(xyz), "voxel")
        got, want = u32(po.cell_start), table_of(name, xyz)
        assert got.shape == want.shape == (512 * grid.leaf_count() + 1,)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"{name} count {count}: cell_start differs in {len(bad)} entries, first at {bad[:4].tolist()}: {got[bad[:4]].tolist()} against {want[bad[:4]].tolist()}"
        assert int(got[-1]) == int(u32(po.leaf_start)[grid.leaf_count()])
        if count == 0:
            assert not got.any()
        assert np.array_equal(u32(po.cell_start), want), "the second call of one sort"
    po.close()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", nc.GRIDS)
def test_neighbours_equal_the_host_mirror(name, rows):
    """every count, every radius and every subset of the outputs, rows behind each output and guard bands watched, the positions only read"""
    grid = dev_grid(name)
    po = device.PointOrder(grid, nc.N_POINTS)
    for count in nc.COUNTS:
        xyz = nc.points(name, count)
        x0 = to_dev(xyz)
        po.sort(x0, "voxel")
        perm = u32(po.perm).astype(np.int64)
        x = po.gather(x0) if rows == "ranked" else x0
        given = u32(x)
        for radius in nc.RADII:
            want = mirror(name, count, radius)
            if rows == "ranked":
                want = tuple(a[perm] for a in want)
            for mask in range(1, 8):
                asked = [k for b, k in enumerate(("count", "density", "push")) if mask >> b & 1]
                slab = outputs(count)
                got = po.neighbours(x, radius, rows=rows, **{k: (slab.views[k][:count] if k in asked else False) for k in ("count", "density", "push")})
                assert sorted(got) == sorted(asked)
                check_outputs(slab, count, asked, want, f"{name} {rows} count {count} radius {radius} outputs {asked}")
        assert u32(x).tobytes() == given.tobytes(), f"{name} {rows} count {count}: the positions were written"
    po.close()


def test_outputs_made_by_the_call():
    name = "ragged32"
    po = device.PointOrder(dev_grid(name), nc.N_POINTS)
    x = to_dev(nc.full_set(name))
    po.sort(x, "voxel")
    got = po.neighbours(x, 1.5)
    nc.same(tuple(u32(got[k]) for k in ("count", "density", "push")), mirror(name, nc.N_POINTS, 1.5), "outputs made by the call")
    assert sorted(po.neighbours(x, 1.5, density=False, push=False)) == ["count"]
    po.close()


def test_a_second_sort_of_other_points_rebuilds_the_table():
    """sort, query, sort other points with another n, query again: a table kept from the first sort would give the first set's ranges"""
    name = "dense32"
    grid = dev_grid(name)
    po = device.PointOrder(grid, nc.N_POINTS)
    first, second = nc.full_set(name), np.ascontiguousarray(nc.full_set(name)[1500:2757][::-1])
    a, b = to_dev(first), to_dev(second)
    po.sort(a, "voxel")
    nc.same(tuple(u32(v) for v in po.neighbours(a, 2.0).values()), mirror(name, nc.N_POINTS, 2.0), "the first sort")
    po.sort(b, "voxel")
    got = po.neighbours(b, 2.0)
    want = leafio.point_neighbours(oc.host_grid(name), second, 2.0)
    assert int(want[0].sum()) >= 1000
    nc.same(tuple(u32(got[k]) for k in ("count", "density", "push")), want, "the second sort")
    assert np.array_equal(u32(po.cell_start), table_of(name, second))
    po.sort(a, "voxel")  # and back, with the larger n
    nc.same(tuple(u32(v) for v in po.neighbours(a, 0.73).values()), mirror(name, nc.N_POINTS, 0.73), "the third sort")
    po.close()


def test_results_do_not_depend_on_what_pooled_memory_held():
    name = "ragged32"
    grid = dev_grid(name)
    xyz = nc.full_set(name)
    want, table = mirror(name, nc.N_POINTS, 2.0), table_of(name, xyz)

    def scenario():
        po = device.PointOrder(grid, nc.N_POINTS + 1000)  # drawn from the pool under the fill, and the table with it
        x = to_dev(xyz)
        po.sort(x, "voxel")
        got = po.neighbours(x, 2.0)
        out = {k: u32(got[k]) for k in ("count", "density", "push")}
        out["cell_start"] = u32(po.cell_start)
        nc.same((out["count"], out["density"], out["push"]), want, "under a fill")
        assert np.array_equal(out["cell_start"], table)
        po.sort(to_dev(xyz[:65]), "voxel")
        out["cell_start_65"] = u32(po.cell_start)
        po.close()
        return out

    pool_cases.under_every_fill(scenario)


def test_sort_and_neighbours_late_on_a_non_blocking_stream():
    """after set_stream to a non-blocking stream, sort, the table and the query run behind a delay, xyz poisoned until its true values arrive on that stream"""
    t = torch()
    name = "dense32"
    grid = dev_grid(name)
    xyz = nc.full_set(name)
    n = len(xyz)
    want, table = mirror(name, n, 2.0), table_of(name, xyz)
    po = device.PointOrder(grid, n)
    x = to_dev(xyz)
    out = {"count": t.empty(n, dtype=t.int32, device="cuda"), "density": t.empty(n, dtype=t.float32, device="cuda"), "push": t.empty((n, 3), dtype=t.float32, device="cuda")}

    def call(stream):
        po.sort(x, "voxel", stream=stream)
        po.neighbours(x, 2.0, **out)
        return {"cell_start": po.cell_start}

    t.cuda.synchronize()
    t0 = time.perf_counter()
    call(0)  # the null stream, device idle before and after: also loads the code objects
    host = time.perf_counter() - t0
    t.cuda.synchronize()
    nc.same(tuple(u32(out[k]) for k in ("count", "density", "push")), want, "null stream")
    delay = sc.Delay(t)
    late = sc.late_call(call, {"xyz": sc.Operand(x, to_dev(xyz))}, dict(out), delay, delay.for_host_time(host), what="neighbours")
    assert late.armed_held
    nc.same(tuple(u32(late.outputs[k]) for k in ("count", "density", "push")), want, "late stream")
    assert np.array_equal(u32(late.outputs["cell_start"]), table)
    sc.assert_inputs_unchanged(late.inputs, {"xyz": xyz}, what="neighbours")
    po.close()


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_refusals_touch_nothing():
    t = torch()
    name, n = "ragged32", 257
    grid = dev_grid(name)
    xyz = nc.points(name, n)
    po = device.PointOrder(grid, 300)
    x = to_dev(xyz)
    c = t.full((300,), 7, dtype=t.int32, device="cuda")
    d, p = t.full((300,), 7.0, device="cuda"), t.full((300, 3), 7.0, device="cuda")
    ptr, table = po._ptr, C.c_void_p(0)
    cells, nbrs = "hns_point_order_cells", "hns_point_order_neighbours"
    query = lambda *a: lib.hns_point_order_neighbours(ptr, *a)
    _refused(lib.hns_point_order_cells(ptr, C.byref(table)), cells, "no sort")
    _refused(query(x.data_ptr(), 0, 1.0, c.data_ptr(), d.data_ptr(), p.data_ptr()), nbrs, "no sort")
    with pytest.raises(RuntimeError, match="no sort"):
        po.cell_start
    with pytest.raises(RuntimeError, match="no sort"):
        po.neighbours(x, 1.0)
    po.sort(x, "leaf")
    _refused(lib.hns_point_order_cells(ptr, C.byref(table)), cells, "level")
    _refused(query(x.data_ptr(), 0, 1.0, c.data_ptr(), d.data_ptr(), p.data_ptr()), nbrs, "level")
    assert table.value is None
    po.sort(x, "voxel")
    before = u32(po.cell_start)
    assert np.array_equal(before, table_of(name, xyz))
    _refused(lib.hns_point_order_cells(ptr, None), cells, "d_cell_start")
    for rows in (-1, 2):
        _refused(query(x.data_ptr(), rows, 1.0, c.data_ptr(), d.data_ptr(), p.data_ptr()), nbrs, "rows")
    for radius in (0.0, -1.0, float("nan"), 2.0000002, float("inf")):
        _refused(query(x.data_ptr(), 0, radius, c.data_ptr(), d.data_ptr(), p.data_ptr()), nbrs, "radius")
    _refused(query(None, 0, 1.0, c.data_ptr(), d.data_ptr(), p.data_ptr()), nbrs, "d_xyz")
    _refused(query(x.data_ptr(), 0, 1.0, None, None, None), nbrs, "all null")
    _refused(query(x.data_ptr(), 0, 1.0, x.data_ptr(), None, None), nbrs, "d_count", "d_xyz")
    _refused(query(x.data_ptr(), 1, 1.0, None, None, x.data_ptr()), nbrs, "d_push", "d_xyz")
    _refused(query(x.data_ptr(), 0, 1.0, c.data_ptr(), c.data_ptr(), None), nbrs, "d_count", "d_density", "same buffer")
    _refused(query(x.data_ptr(), 0, 1.0, None, d.data_ptr(), d.data_ptr()), nbrs, "d_density", "d_push", "same buffer")
    with pytest.raises(ValueError, match="rows"):
        po.neighbours(x, 1.0, rows="sorted")
    with pytest.raises(ValueError, match="none of"):
        po.neighbours(x, 1.0, count=False, density=False, push=False)
    with pytest.raises(ValueError, match="rows"):
        po.neighbours(x[:200], 1.0)
    with pytest.raises(ValueError, match="density must be"):
        po.neighbours(x, 1.0, density=d)
    with pytest.raises(ValueError, match="radius"):
        po.neighbours(x, 2.5)
    t.cuda.synchronize()
    assert bool((c == 7).all()) and bool((d == 7.0).all()) and bool((p == 7.0).all()) and u32(x).tobytes() == xyz.view(np.uint32).tobytes()
    assert np.array_equal(u32(po.cell_start), before)
    nc.same(tuple(u32(v) for v in po.neighbours(x, 1.0).values()), mirror(name, n, 1.0), "after the refusals")
    po.close()
    for use in (lambda: po.cell_start, lambda: po.neighbours(x, 1.0)):
        with pytest.raises(RuntimeError, match="closed"):
            use()


def test_no_points_launch_nothing():
    t = torch()
    grid = dev_grid("ragged32")
    po = device.PointOrder(grid, 16)
    po.sort(t.zeros((0, 3), device="cuda"), "voxel")
    assert not u32(po.cell_start).any() and len(u32(po.cell_start)) == 512 * grid.leaf_count() + 1
    got = po.neighbours(t.zeros((0, 3), device="cuda"), 1.0)
    assert [tuple(got[k].shape) for k in ("count", "density", "push")] == [(0,), (0,), (0, 3)]
    assert lib.hns_point_order_neighbours(po._ptr, None, 0, 1.0, None, 256, None) == _lib.HNS_OK  # no pointer is looked at: this one is no device address
    t.cuda.synchronize()
    po.close()
