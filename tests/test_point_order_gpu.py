"""The leaf order of a point set on the GPU: device.PointOrder (hns_point_order_*: the radix sort, the ranges and the row moves of hns_pointorder.hip) against the host
mirror leafio.sort_points, which tests/test_point_order.py holds to the numpy restatement. Every comparison is equality of bytes: the result of a stable sort is unique.
Grids, point sets and their conditions are tests/order_cases.py's; the tile and scan boundaries come from the constants the Python layer exposes."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import order_cases as oc
import pool_cases
import seed_cases as sd
import stream_cases as sc
from frame_cases import LAUNCH_RANGES, launch_range, make_sim, random_state
from hnanosolver_amd import _lib, api, device, fields, leafio
from hnanosolver_amd._lib import lib

pytestmark = pytest.mark.gpu

F = np.float32
T, S = device.POINT_ORDER_TILE, device.POINT_ORDER_SCAN_TILES
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


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


def results(po):
    return u32(po.perm), u32(po.keys), u32(po.leaf_start)


def sort_and_check(po, grid, xyz, level, what):
    """one device sort of xyz against the host mirror on the same grid, stability stated directly, xyz only read -> the device's (perm, keys, leaf_start)"""
    x = to_dev(xyz)
    po.sort(x, oc.LEVEL_NAMES[level])
    got = results(po)
    assert po.n == len(xyz) and len(got[0]) == len(xyz) and len(got[2]) == grid.leaf_count() + 3
    oc.same(got, leafio.sort_points(grid, xyz, level), what)
    oc.assert_stable_permutation(got[0], got[1], what)
    assert x.cpu().numpy().tobytes() == np.ascontiguousarray(xyz, dtype=F).tobytes(), f"{what}: xyz was written"
    return got


def scattered_points(n, seed, lo=-8.0, hi=72.0):
    """n points uniform over a box around the 64^3 grid (a quarter outside), a NaN or an inf every 997th: cheap to make in the millions"""
    rng = np.random.default_rng([seed, 9])
    x = rng.uniform(lo, hi, (n, 3)).astype(F)
    x[::997, 1] = F(np.nan)
    x[500::1994, 2] = F(np.inf)
    return x


@pytest.mark.parametrize("level", oc.LEVELS)
@pytest.mark.parametrize("name", oc.GRIDS)
def test_grids_levels_and_counts(name, level):
    grid = dev_grid(name)
    po = device.PointOrder(grid, len(oc.full_set(name)))
    for count in oc.COUNTS:
        xyz = oc.points(name, count)
        what = f"{name} level {level} count {count}"
        first = sort_and_check(po, grid, xyz, level, what)
        oc.same(sort_and_check(po, grid, xyz, level, what + " (again)"), first, what + ": the second sort of the same object")
    po.close()


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_every_leaf_is_a_bin_whatever_the_launch_range(kind):
    """include/hns.h: the order counts every leaf whatever the grid's launch range, ghost leaves included -- an object made before the range was narrowed and one made
    under it give the whole range's permutation, keys and leaf ranges (which equal the host mirror) under set_active_range on a strict inner range and under
    set_active_leaves(n // 2)"""
    name = "ragged32"
    grid, xyz = dev_grid(name), oc.full_set(name)
    po = device.PointOrder(grid, len(xyz))
    for level in oc.LEVELS:
        whole = sort_and_check(po, grid, xyz, level, f"whole range, level {level}")
        with launch_range(grid, kind):
            x = to_dev(xyz)
            po.sort(x, oc.LEVEL_NAMES[level])
            got = results(po)
            fresh = device.PointOrder(grid, len(xyz))
            fresh.sort(x, oc.LEVEL_NAMES[level])
            got_fresh, ranked = results(fresh), u32(fresh.gather(x))
            fresh.close()
        assert grid.active_leaves() == grid.leaf_count()
        oc.same(got, whole, f"{kind}, level {level}")
        oc.same(got_fresh, whole, f"{kind}, level {level}, an object made under the range")
        assert np.array_equal(ranked, np.ascontiguousarray(xyz).view(np.uint32)[whole[0]]), f"{kind}, level {level}: gather"
    po.close()


def passes_of(n_leaves, level):
    top = 512 * (n_leaves + 1) if level else n_leaves + 1
    return max(1, -(-top.bit_length() // 8))


@pytest.mark.parametrize("name,level,passes", [("one_leaf", 0, 1), ("dense64", 0, 2), ("dense64", 1, 3)])
def test_pass_counts_one_to_three(name, level, passes):
    assert passes_of(len(oc.origins(name)), level) == passes
    grid, xyz = dev_grid(name), oc.full_set(name)
    po = device.PointOrder(grid, len(xyz))
    sort_and_check(po, grid, xyz, level, f"{name} level {level}: {passes} passes")
    po.close()


def test_four_passes_on_a_256_cube():
    """a 256^3 dense topology at voxel level: (32768 + 2) * 512 > 2^24. Only the grid is built; no field is allocated"""
    o = np.ascontiguousarray(fields.dense_leaves(256), dtype=np.int32)
    assert len(o) == 32768 and passes_of(len(o), 1) == 4 and passes_of(len(o), 0) == 2
    grid = api.create_grid_from_leaves(o, oc.VS)
    xyz = np.concatenate([scattered_points(100003, 4, -16.0, 272.0), sd.edges()])
    po = device.PointOrder(grid, len(xyz))
    got = sort_and_check(po, grid, xyz, 1, "256^3 level 1")
    assert int(got[1].max()) >= 1 << 24  # (the fourth digit is not all zero)
    sort_and_check(po, grid, xyz, 0, "256^3 level 0")
    po.close()
    grid.reset()


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1, T * S + 1], ids=["tile-1", "tile", "tile+1", "2tiles+1", "scan_chunk+1"])
def test_tile_and_scan_boundaries(n):
    grid = dev_grid("dense64")
    xyz = scattered_points(n, n % 1000)
    po = device.PointOrder(grid, n)
    for level in oc.LEVELS if n < T * S else (1,):
        sort_and_check(po, grid, xyz, level, f"{n} points level {level}")
    po.close()


@pytest.mark.parametrize("level", oc.LEVELS)
@pytest.mark.parametrize("kind", oc.DISTRIBUTIONS)
def test_adversarial_distributions(kind, level):
    grid = dev_grid("dense64")
    xyz = oc.distribution(kind)
    po = device.PointOrder(grid, len(xyz))
    got = sort_and_check(po, grid, xyz, level, f"{kind} level {level}")
    if kind == "sorted" and level == 1:
        assert np.array_equal(got[0], np.arange(len(xyz), dtype=np.uint32))
    po.close()


def test_reuse_larger_smaller_empty():
    """n = capacity, a small n, 0, capacity again on one object: nothing of an earlier sort survives"""
    grid = dev_grid("dense64")
    cap = 2 * T + 77
    po = device.PointOrder(grid, cap)
    big, other = scattered_points(cap, 1), scattered_points(cap, 2)
    sort_and_check(po, grid, big, 1, "capacity")
    sort_and_check(po, grid, oc.points("dense64", 65), 0, "65 behind capacity")
    sort_and_check(po, grid, np.zeros((0, 3), dtype=F), 1, "0 behind 65")
    assert not u32(po.leaf_start).any() and len(u32(po.perm)) == 0
    sort_and_check(po, grid, other, 1, "capacity behind 0")
    sort_and_check(po, grid, big[: T + 1], 1, "a tile and one")
    po.close()


@pytest.mark.parametrize("row_bytes", [4, 12, 16, 64])
def test_rows_gather_and_scatter_inside_guard_bands(row_bytes):
    t = torch()
    grid, W = dev_grid("dense64"), row_bytes // 4
    xyz = oc.full_set("dense64")
    n, extra = len(xyz), 5
    po = device.PointOrder(grid, n)
    po.sort(to_dev(xyz), "voxel")
    perm = u32(po.perm).astype(np.int64)
    rng = np.random.default_rng(row_bytes)
    x = rng.integers(0, 2 ** 32, (n, W), dtype=np.uint64).astype(np.uint32).view(F)  # any 32-bit words, NaN patterns included
    src = to_dev(x) if W > 1 else to_dev(x.reshape(n))
    shape = (n + extra, W) if W > 1 else (n + extra,)
    slab = sc.Slab(t, {"gathered": (shape, F), "back": (shape, F)}, device="cuda")
    for v in slab.views.values():
        sc.sentinel(v)
    assert po.gather(src, slab.views.gathered) is slab.views.gathered
    po.scatter(slab.views.gathered, slab.views.back)
    t.cuda.synchronize()
    slab.check(f"rows of {row_bytes} bytes")
    g, b = (u32(slab.views[k]).reshape(n + extra, W) for k in ("gathered", "back"))
    xw = x.view(np.uint32).reshape(n, W)
    assert np.array_equal(g[:n], xw[perm]), "gather is not x[perm]"
    assert np.array_equal(b[:n], xw), "scatter(gather(x)) is not x"
    assert (g[n:] == sc.OUT_WORD).all() and (b[n:] == sc.OUT_WORD).all(), "rows behind n were written"
    assert u32(src).tobytes() == xw.tobytes()
    made = po.gather(src)  # (a destination made by the call: n rows)
    assert tuple(made.shape) == tuple(src.shape) and np.array_equal(u32(made).reshape(n, W), xw[perm])
    po.close()


def test_point_calls_on_gathered_points_scattered_back():
    """what the order is for: sample_points, trace_points (order 4, 3 steps, status) and splat_points on the gathered points give what they give on the original order"""
    t = torch()
    grid, o = dev_grid("dense64"), oc.origins("dense64")
    xyz = oc.full_set("dense64")
    n = len(xyz)
    rng = np.random.default_rng(17)
    vel = to_dev(rng.standard_normal((len(o) * 512, 3)).astype(F))
    phi = to_dev(rng.standard_normal(len(o) * 512).astype(F))
    po = device.PointOrder(grid, n)
    x0 = to_dev(xyz)
    po.sort(x0, "voxel")
    xs = po.gather(x0)
    # sample
    want = device.sample_points(grid, [phi, vel], x0)
    got = [po.scatter(s) for s in device.sample_points(grid, [phi, vel], xs)]
    for a, b, what in zip(got, want, ("float", "Vec3f")):
        assert u32(a).tobytes() == u32(b).tobytes(), f"sample_points: the {what} field"
    # trace
    pa, pb = x0.clone(), xs.clone()
    sa, sb = (t.full((n,), 0xAB, dtype=t.uint8, device="cuda") for _ in range(2))
    device.trace_points(grid, vel, pa, 0.04, 24.0, order=4, steps=3, status=sa)
    device.trace_points(grid, vel, pb, 0.04, 24.0, order=4, steps=3, status=sb)
    assert u32(po.scatter(pb)).tobytes() == u32(pa).tobytes(), "trace_points: positions"
    assert u32(po.scatter(sb.to(t.int32))).tobytes() == u32(sa.to(t.int32)).tobytes(), "trace_points: status"
    # splat
    values = to_dev(rng.standard_normal(n).astype(F))
    fa, fb = phi.clone(), phi.clone()
    device.splat_points(grid, [fa], x0, [values])
    device.splat_points(grid, [fb], xs, [po.gather(values)])
    assert u32(fa).tobytes() == u32(fb).tobytes() and u32(fa).tobytes() != u32(phi).tobytes(), "splat_points: field bytes"
    po.close()


def test_results_do_not_depend_on_what_pooled_memory_held():
    grid = dev_grid("ragged32")
    xyz = oc.full_set("ragged32")
    rows = np.random.default_rng(2).standard_normal((len(xyz), 3)).astype(F)
    want = leafio.sort_points(grid, xyz, "voxel")

    def scenario():
        po = device.PointOrder(grid, len(xyz) + 1000)  # drawn from the pool under the fill
        po.sort(to_dev(xyz), "voxel")
        got = results(po)
        oc.same(got, want, "under a fill")
        out = {"perm": got[0], "keys": got[1], "leaf_start": got[2], "rows": po.gather(to_dev(rows)).cpu().numpy()}
        po.sort(to_dev(xyz[:65]), "leaf")
        out["leaf_start_65"] = u32(po.leaf_start)
        po.close()
        return out

    pool_cases.under_every_fill(scenario)


def test_sort_and_gather_late_on_a_non_blocking_stream():
    """after set_stream to a non-blocking stream, sort then gather run behind a delay, xyz and the rows poisoned until their true values arrive on that stream"""
    t = torch()
    grid = dev_grid("dense64")
    xyz = oc.full_set("dense64")
    n = len(xyz)
    rows = np.random.default_rng(3).standard_normal((n, 4)).astype(F)
    want = leafio.sort_points(grid, xyz, "voxel")
    po = device.PointOrder(grid, n)
    x, r = to_dev(xyz), to_dev(rows)
    out = t.empty((n, 4), dtype=t.float32, device="cuda")

    def call(stream):
        po.sort(x, "voxel", stream=stream)
        po.gather(r, out)
        return {"perm": po.perm, "keys": po.keys, "leaf_start": po.leaf_start}

    t.cuda.synchronize()
    t0 = time.perf_counter()
    call(0)  # the null stream, device idle before and after: also loads the code objects
    host = time.perf_counter() - t0
    t.cuda.synchronize()
    oc.same(results(po), want, "null stream")
    null_rows = u32(out)
    delay = sc.Delay(t)
    late = sc.late_call(call, {"xyz": sc.Operand(x, to_dev(xyz)), "rows": sc.Operand(r, to_dev(rows))}, {"gathered": out}, delay, delay.for_host_time(host), what="point order")
    assert late.armed_held
    oc.same(tuple(u32(late.outputs[k]) for k in ("perm", "keys", "leaf_start")), want, "late stream")
    assert u32(late.outputs["gathered"]).tobytes() == null_rows.tobytes() == rows.view(np.uint32)[want[0].astype(np.int64)].tobytes()
    sc.assert_inputs_unchanged(late.inputs, {"xyz": xyz, "rows": rows}, what="point order")
    po.close()


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_refusals_touch_nothing():
    t = torch()
    grid = dev_grid("ragged32")
    xyz = oc.points("ragged32", 257)
    po = device.PointOrder(grid, 300)
    x = to_dev(xyz)
    a, b = (t.full((300, 3), 7.0, device="cuda") for _ in range(2))
    p = po._ptr
    _refused(lib.hns_point_order_gather(p, a.data_ptr(), b.data_ptr(), 12), "hns_point_order_gather", "no sort")
    _refused(lib.hns_point_order_scatter(p, a.data_ptr(), b.data_ptr(), 12), "hns_point_order_scatter", "no sort")
    with pytest.raises(RuntimeError, match="no sort"):
        po.gather(a)
    info = _lib.hns_point_order_info()
    assert lib.hns_point_order_get(p, C.byref(info)) == 0 and (info.n, info.level, info.capacity, info.n_leaves) == (0, -1, 300, 32)
    _refused(lib.hns_point_order_sort(p, x.data_ptr(), 301, 1), "hns_point_order_sort", "capacity")
    _refused(lib.hns_point_order_sort(p, x.data_ptr(), 2 ** 31, 1), "hns_point_order_sort", "n is above")
    _refused(lib.hns_point_order_sort(p, x.data_ptr(), 257, 2), "hns_point_order_sort", "level")
    _refused(lib.hns_point_order_sort(p, None, 257, 1), "hns_point_order_sort", "xyz")
    _refused(lib.hns_point_order_gather(p, a.data_ptr(), b.data_ptr(), 12), "hns_point_order_gather", "no sort")  # (a refused sort is no sort)
    with pytest.raises(ValueError, match="capacity"):
        po.sort(t.zeros((301, 3), device="cuda"))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        po.sort(t.zeros((30, 4), device="cuda"))
    po.sort(x, "voxel")
    want = results(po)
    for bad in (0, 2, 6, 68, -4):
        _refused(lib.hns_point_order_gather(p, a.data_ptr(), b.data_ptr(), bad), "hns_point_order_gather", "row_bytes")
    _refused(lib.hns_point_order_gather(p, a.data_ptr(), a.data_ptr(), 12), "hns_point_order_gather", "same buffer")
    _refused(lib.hns_point_order_scatter(p, a.data_ptr(), a.data_ptr(), 12), "hns_point_order_scatter", "same buffer")
    _refused(lib.hns_point_order_scatter(p, None, b.data_ptr(), 12), "hns_point_order_scatter", "null")
    _refused(lib.hns_point_order_sort(p, x.data_ptr(), 257, -1), "hns_point_order_sort", "level")
    with pytest.raises(ValueError, match="row of src"):
        po.gather(t.zeros((257, 17), device="cuda"))
    with pytest.raises(ValueError, match="rows"):
        po.gather(t.zeros((256, 3), device="cuda"))
    with pytest.raises(ValueError, match="dst rows"):
        po.gather(a, t.zeros((300, 4), device="cuda"))
    t.cuda.synchronize()
    assert bool((a == 7.0).all()) and bool((b == 7.0).all())
    oc.same(results(po), want, "after the refusals")  # (a refused sort leaves the last one's results)
    err = C.c_int(0)
    host_only = oc.host_grid("ragged32")
    assert lib.hns_point_order_create(host_only.ptr, 16, C.byref(err)) is None
    _refused(err.value, "hns_point_order_create", "HNS_GRID_HOST_ONLY")
    po.close()
    po.close()
    for use in (lambda: po.sort(x), lambda: po.perm, lambda: po.gather(a), lambda: po.scatter(a)):
        with pytest.raises(RuntimeError, match="closed"):
            use()


def test_sim_point_order_refuses_after_a_regrid():
    o = oc.origins("ragged32")
    names = ["density"]
    g, sim = make_sim(o, names, random_state(5, len(o), names))
    xyz = oc.points("ragged32", 257)
    x = to_dev(xyz)
    po = sim.point_order(300)
    assert po.grid is g
    po.sort(x, "leaf")
    oc.same(results(po), leafio.sort_points(g, xyz, "leaf"), "on the sim's grid")
    new = sim.regrid(1)
    assert sim.grid is new and new is not g
    for use in (lambda: po.sort(x), lambda: po.perm, lambda: po.gather(x)):
        with pytest.raises(RuntimeError, match="regrid"):
            use()
    po.close()
    fresh = sim.point_order(300)
    fresh.sort(x, "leaf")
    oc.same(results(fresh), leafio.sort_points(new, xyz, "leaf"), "on the sim's new grid")
    fresh.close()
    sim.close()
