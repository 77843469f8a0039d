"""The leaf order of a point set without a GPU: the host mirror hns_grid_sort_points (leafio.sort_points) against the numpy restatement of tests/order_cases.py, bytes of
perm, keys and leaf_start; the conditions the point sets must meet, on the restatement's count; the refusals of the C ABI that need no device; and the argument checks of
the Python layer. tests/test_point_order_gpu.py holds the device's sort to the same mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import order_cases as oc
from hnanosolver_amd import _lib, device, leafio
from hnanosolver_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", oc.GRIDS)
def test_point_sets_meet_their_conditions(name):
    g, L = oc.host_grid(name), len(oc.origins(name))
    xyz = oc.full_set(name)
    assert len(xyz) == 4099 + 61
    inside, outside, unsorted = oc.shares(g, L, xyz)
    print(f"{name}: in a leaf {inside:.3f}, outside {outside:.3f}, {unsorted} do not sort")
    assert inside >= 0.50 and outside >= 0.25 and unsorted >= 15, (name, inside, outside, unsorted)


def test_the_512_leaf_set_leaves_leaves_empty():
    g, L = oc.host_grid("dense64"), len(oc.origins("dense64"))
    assert L == 512
    _, _, leaf_start = oc.restate(g, L, oc.full_set("dense64"), 0)
    per_leaf = np.diff(leaf_start.astype(np.int64))[:L]
    hit, empty = int((per_leaf > 0).sum()), int((per_leaf == 0).sum())
    print(f"dense64: {hit} leaves hit, {empty} empty")
    assert empty >= 1 and hit >= 400


@pytest.mark.parametrize("count", oc.COUNTS)
@pytest.mark.parametrize("level", oc.LEVELS)
@pytest.mark.parametrize("name", oc.GRIDS)
def test_host_mirror_matches_the_restatement(name, level, count):
    g, L = oc.host_grid(name), len(oc.origins(name))
    xyz = oc.points(name, count)
    before = xyz.copy()
    got = leafio.sort_points(g, xyz, oc.LEVEL_NAMES[level])
    assert all(a.dtype == np.uint32 for a in got) and len(got[2]) == L + 3
    oc.same(got, oc.restate(g, L, xyz, level), f"{name} level {level} count {count}")
    oc.assert_stable_permutation(got[0], got[1], f"{name} level {level} count {count}")
    assert int(got[2][0]) == 0 and int(got[2][-1]) == len(xyz)
    assert xyz.tobytes() == before.tobytes()


@pytest.mark.parametrize("kind", oc.DISTRIBUTIONS)
def test_host_mirror_on_the_adversarial_distributions(kind):
    g, L = oc.host_grid("dense64"), 512
    xyz = oc.distribution(kind)
    assert len(xyz) == oc.N_BIG
    for level in oc.LEVELS:
        got = leafio.sort_points(g, xyz, level)
        oc.same(got, oc.restate(g, L, xyz, level), f"{kind} level {level}")
    inside, outside, unsorted = oc.shares(g, L, xyz)
    want = {"all_outside": (0.0, 1.0, 0), "all_nan": (0.0, 0.0, oc.N_BIG), "one_voxel": (1.0, 0.0, 0), "alternating": (1.0, 0.0, 0)}.get(kind)
    if want:
        assert (inside, outside, unsorted) == want, (kind, inside, outside, unsorted)
    if kind == "sorted":
        assert np.array_equal(got[0], np.arange(oc.N_BIG, dtype=np.uint32))
    if kind == "corner_ball":
        assert int((np.diff(got[2].astype(np.int64))[:L] > 0).sum()) == 8


def test_keys_and_ranges_may_be_left_out():
    g = oc.host_grid("ragged32")
    xyz = oc.points("ragged32", 257)
    perm = np.zeros(257, dtype=np.uint32)
    _lib.check(lib.hns_grid_sort_points(g.ptr, xyz.ctypes.data, 257, 1, perm.ctypes.data, None, None))
    assert np.array_equal(perm, leafio.sort_points(g, xyz, "voxel")[0])


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_host_mirror_refusals_touch_nothing():
    g = oc.host_grid("ragged32")
    xyz = oc.points("ragged32", 64)
    perm, keys, ls = (np.full(k, 0xDEADBEEF, dtype=np.uint32) for k in (64, 64, 35))
    args = (perm.ctypes.data, keys.ctypes.data, ls.ctypes.data)
    _refused(lib.hns_grid_sort_points(None, xyz.ctypes.data, 64, 1, *args), "hns_grid_sort_points", "grid")
    _refused(lib.hns_grid_sort_points(g.ptr, None, 64, 1, *args), "hns_grid_sort_points", "xyz")
    _refused(lib.hns_grid_sort_points(g.ptr, xyz.ctypes.data, 2 ** 31, 1, *args), "hns_grid_sort_points", "n is above")
    _refused(lib.hns_grid_sort_points(g.ptr, xyz.ctypes.data, 64, 2, *args), "hns_grid_sort_points", "level")
    _refused(lib.hns_grid_sort_points(g.ptr, xyz.ctypes.data, 64, -1, *args), "hns_grid_sort_points", "level")
    _refused(lib.hns_grid_sort_points(g.ptr, xyz.ctypes.data, 64, 1, None, keys.ctypes.data, ls.ctypes.data), "hns_grid_sort_points", "perm")
    for a in (perm, keys, ls):
        assert (a == 0xDEADBEEF).all()
    assert lib.hns_grid_sort_points(g.ptr, None, 0, 0, None, None, ls.ctypes.data) == _lib.HNS_OK and not ls.any()  # n == 0: nothing is looked at, the ranges are all zero


def test_object_refusals_that_need_no_device():
    g = oc.host_grid("ragged32")
    err = C.c_int(7)
    assert lib.hns_point_order_create(None, 16, C.byref(err)) is None
    _refused(err.value, "hns_point_order_create", "grid")
    err = C.c_int(7)
    assert lib.hns_point_order_create(g.ptr, 2 ** 31, C.byref(err)) is None
    _refused(err.value, "hns_point_order_create", "capacity")
    err = C.c_int(7)
    assert lib.hns_point_order_create(g.ptr, 16, C.byref(err)) is None  # a host-only grid: no device here, or no device tables there
    text = lib.hns_last_error().decode()
    if lib.hns_device_count() == 0:
        assert err.value == _lib.HNS_ERR_NO_DEVICE and "hns_point_order_create" in text and "no HIP device" in text
    else:
        _refused(err.value, "hns_point_order_create", "HNS_GRID_HOST_ONLY")
    assert lib.hns_point_order_create(None, 16, None) is None  # (err may be null)
    info = _lib.hns_point_order_info()
    _refused(lib.hns_point_order_set_stream(None, None), "hns_point_order_set_stream", "null point order")
    _refused(lib.hns_point_order_sort(None, None, 0, 1), "hns_point_order_sort", "null point order")
    _refused(lib.hns_point_order_get(None, C.byref(info)), "hns_point_order_get", "null point order")
    _refused(lib.hns_point_order_gather(None, None, None, 4), "hns_point_order_gather", "null point order")
    _refused(lib.hns_point_order_scatter(None, None, None, 4), "hns_point_order_scatter", "null point order")
    lib.hns_point_order_destroy(None)


def test_python_layer_argument_checks():
    g = oc.host_grid("ragged32")
    xyz = oc.points("ragged32", 64)
    for bad in ("cell", 2, -1, None, True, 1.0):
        with pytest.raises(ValueError, match="level"):
            leafio.sort_points(g, xyz, bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        leafio.sort_points(g, xyz.reshape(-1), "voxel")
    assert leafio.sort_level("leaf") == 0 and leafio.sort_level("voxel") == 1 and leafio.sort_level(0) == 0 and leafio.sort_level(np.int64(1)) == 1
    with pytest.raises(ValueError, match="negative"):
        device.PointOrder(g, -1)
    with pytest.raises((_lib.HNSError, ValueError)) as e:  # a host-only grid has no device side
        device.PointOrder(g, 16)
    # (without a device the refusal is HNS_ERR_NO_DEVICE, an HNSError; with one it is HNS_ERR_INVALID_ARGUMENT, which the Python layer raises as ValueError)
    assert getattr(e.value, "code", BAD) in (_lib.HNS_ERR_NO_DEVICE, BAD) and "hns_point_order_create" in str(e.value)


def test_python_constants_are_the_kernels():
    """device.POINT_ORDER_TILE and POINT_ORDER_SCAN_TILES, from which the GPU tests take their boundary counts, are the constants of hns_pointorder.hip"""
    src = open(os.path.join(ROOT, "hnanosolver_amd", "csrc", "hns_pointorder.hip")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    assert device.POINT_ORDER_TILE == value("kOrderBlock") * value("kOrderItems")
    assert device.POINT_ORDER_SCAN_TILES == value("kOrderBlock") * value("kScanItems")
    assert re.search(r"constexpr int kOrderTile = kOrderBlock \* kOrderItems;", src) and re.search(r"constexpr int kScanChunk = kOrderBlock \* kScanItems;", src)
