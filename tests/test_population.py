"""Birth and death of points without a GPU: the host mirror hns_grid_birth_points (leafio.birth_points) against the numpy restatement of tests/population_cases.py, every
byte, live and wanted included; the conditions the inputs must meet, on the restatement's count; the properties of a birth; the refusals of the C ABI that need no device;
the constants and the kernel resources of hns_population.hip. tests/test_population_gpu.py holds the device's select, compact and birth to the same mirror."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import population_cases as P
from hnanosolver_amd import _lib, api, device, leafio
from hnanosolver_amd._lib import lib
from test_kernel_resources import CSRC, HIPCC, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _lib.HNS_ERR_INVALID_ARGUMENT
F, U32 = np.float32, np.uint32
NEW = ("hns_point_population_create", "hns_point_population_destroy", "hns_point_population_set_stream", "hns_point_population_set_live", "hns_point_population_select",
       "hns_point_population_compact", "hns_point_population_birth", "hns_point_population_birth_sim", "hns_point_population_get", "hns_point_population_counts",
       "hns_grid_birth_points")


def test_every_new_symbol_is_exported_declared_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hns_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hns.h")).read(), flags=re.S)
    for name in NEW:
        assert name in exported, f"{name} is not exported"
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/hns.h"
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], f"{name} is not bound"
    assert not any("stream" in re.search(name + r"\s*\(([^;]*)\);", header, flags=re.S).group(1).replace("hip_stream", "") for name in NEW)  # (the stream is bound once)
    assert lib.hns_version() == 100
    assert C.sizeof(_lib.hns_birth_spec) == 20 and C.sizeof(_lib.hns_point_population_info) == 32


def counts_of(grid_name, kind):
    v, m, spec = P.case(grid_name, kind)
    return P.counts(P.origins(grid_name), v, m, spec["threshold"], spec["rate"], spec["max_per_voxel"], spec["seed"])


@pytest.mark.parametrize("kind", P.FIELDS)
@pytest.mark.parametrize("grid_name", P.GRIDS)
def test_host_mirror_matches_the_restatement(grid_name, kind):
    o, g = P.origins(grid_name), P.host_grid(grid_name)
    v, m, spec = P.case(grid_name, kind)
    before = v.copy()
    c = counts_of(grid_name, kind)[0]
    cases = P.capacities(c)
    assert {"zero_rows", "exact", "roomy_filled", "roomy_kept", "appended"} <= set(cases)
    for name, (rows, start, fill) in cases.items():
        sx, sv = P.sentinels(rows)
        got = leafio.birth_points(g, v, m, **spec, fill=fill, start=start, capacity_rows=rows, xyz=sx, voxel=sv)
        want = P.restate_birth(o, v, m, **spec, fill=fill, start=start, capacity_rows=rows)
        P.same_birth(got, want, f"{grid_name} {kind} {name}")
        assert want[3] == start + int(c.sum()) and want[2] == min(want[3], rows)
    assert v.tobytes() == before.tobytes()
    if kind == "zero":
        assert int(c.sum()) == 0 and counts_of(grid_name, kind)[2].sum() >= 512  # eligible voxels that bear nothing
    if kind == "saturated":
        in_range = ((P.coordinates(o) >= -8388608) & (P.coordinates(o) <= 8388606)).all(1)
        assert (c[in_range] == 16).all() and (c[~in_range] == 0).all()
        assert grid_name != "one_leaf" or int(c.sum()) == 8192
    if kind == "at_threshold":
        at = np.asarray(v) == F(spec["threshold"])
        assert at.sum() >= 100 and not c[at].any() and c[np.asarray(v) == np.nextafter(F(spec["threshold"]), F(np.inf))].any()
    if kind == "masked" and len(o) > 1:
        off = ~P.mask_bits(m, len(o))
        assert off.sum() >= 512 and not c[off].any() and (np.asarray(v)[off] * F(spec["rate"]) >= 1).any()  # bits cleared over voxels that would bear
    if "cut_inside_a_run" in cases:
        rows = cases["cut_inside_a_run"][0]
        ends = np.cumsum(c)
        assert not (ends == rows).any() and rows < ends[-1], "the cut lies on a voxel boundary"


def test_the_random_case_meets_its_conditions():
    """dense64, K = 4: every count value occurs in at least 5 % of the voxels, and the fractions round up about as often as they are large"""
    c, h, eligible, f = counts_of("dense64", "random")
    shares = np.bincount(c, minlength=5) / len(c)
    print("count shares", shares.round(3).tolist())
    assert len(shares) == 5 and (shares >= 0.05).all(), shares
    frac = eligible & (f > 0)
    b = np.floor(np.minimum(np.where(eligible, P.case("dense64", "random")[0], F(0)) * F(2.5), F(4))).astype(np.int64)
    up = float((c[frac] > b[frac]).mean())
    print(f"round-up share {up:.3f} at a mean f of {float(f[frac].mean()):.3f} over {int(frac.sum())} voxels")
    assert 0.4 <= up <= 0.6
    v = np.asarray(P.case("dense64", "random")[0])
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (np.signbit(v) & (v == 0)).any() and (v < -1).any()
    assert not c[np.isnan(v)].any() and (c[np.isposinf(v)] == 4).all()


def test_a_coordinate_is_clamped_where_floats_are_coarse():
    for grid_name, kind in (("sparse_far", "saturated"), ("range_edge", "random")):
        v, m, spec = P.case(grid_name, kind)
        xyz, e, clamped, _ = P.births(P.origins(grid_name), v, m, spec["threshold"], spec["rate"], spec["max_per_voxel"], spec["seed"])
        print(f"{grid_name}: {int(clamped.sum())} clamped coordinates of {3 * len(xyz)}")
        assert clamped.any()
        i = P.coordinates(P.origins(grid_name))[e.astype(np.int64)]
        assert (xyz[clamped] == np.nextafter((i[clamped] + 1).astype(F), F(-np.inf))).all() and (np.floor(xyz.astype(np.float64)) == i).all()


@pytest.mark.parametrize("grid_name", P.GRIDS)
def test_every_birth_lies_in_its_voxel(grid_name):
    o, g = P.origins(grid_name), P.host_grid(grid_name)
    kind = "saturated" if grid_name in ("one_leaf", "sparse_far") else "random"
    v, m, spec = P.case(grid_name, kind)
    wanted = int(counts_of(grid_name, kind)[0].sum())
    xyz, voxel, live, _ = leafio.birth_points(g, v, m, **spec, capacity_rows=wanted)
    assert live == wanted > 0
    cell = np.floor(xyz.astype(np.float64)).astype(np.int32)
    assert np.array_equal(cell, P.coordinates(o)[voxel.astype(np.int64)])
    assert np.array_equal(g.offsets(cell).astype(np.int64), voxel.astype(np.int64) + 1)
    assert (np.diff(voxel.astype(np.int64)) >= 0).all()  # voxel order
    from seed_cases import seeding
    assert seeding(xyz).all()  # every birth meets the seeds' condition


def test_a_voxel_bears_the_same_points_on_any_grid_that_holds_it():
    """the leaves of five_leaves in another order among extra leaves, the field carried along: the shared voxels bear the same positions"""
    o5, o64 = P.origins("five_leaves"), P.origins("dense64")
    pick = np.array([300, 4, 17, 0, 2, 511, 1, 3])
    other = api.create_grid_from_leaves(np.ascontiguousarray(o64[pick]), 1.0 / 24.0, _lib.HNS_GRID_HOST_ONLY)
    v64 = P.random_field("dense64").reshape(-1, 512)
    spec = dict(P.SPEC)
    a = leafio.birth_points(P.host_grid("five_leaves"), v64[:5], **spec, capacity_rows=20000)
    b = leafio.birth_points(other, v64[pick], **spec, capacity_rows=20000)
    assert a[2] == a[3] and b[2] == b[3] and a[2] > 1000
    shared = np.isin(pick[b[1][: b[2]].astype(np.int64) >> 9], np.arange(5))
    rows = lambda x: sorted(map(bytes, np.ascontiguousarray(x).view(np.uint8).reshape(len(x), 12)))
    assert rows(a[0][: a[2]]) == rows(b[0][: b[2]][shared]) and shared.sum() == a[2]
    assert np.array_equal(o5, o64[:5])


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_host_mirror_refusals_touch_nothing():
    g = P.host_grid("one_leaf")
    v = np.full(512, 1.0, dtype=F)
    xyz, voxel = P.sentinels(64)
    live, wanted = C.c_uint64(77), C.c_uint64(78)
    who = "hns_grid_birth_points"

    def call(grid=g.ptr, field=v.ctypes.data, spec=None, x=xyz.ctypes.data, vox=voxel.ctypes.data, rows=64, null_spec=False, **changes):
        s = leafio.birth_spec(**{**dict(threshold=0.25, rate=2.5, max_per_voxel=4, seed=1), **changes})
        return lib.hns_grid_birth_points(grid, field, None, None if null_spec else C.byref(s), 0, x, vox, rows, C.byref(live), C.byref(wanted))

    _refused(call(grid=None), who, "grid")
    _refused(call(field=None), who, "field")
    _refused(call(null_spec=True), who, "spec")
    _refused(call(x=None), who, "xyz")
    _refused(call(rows=2 ** 31), who, "capacity_rows")
    for k in (0, 17, 2 ** 31):
        _refused(call(max_per_voxel=k), who, "max_per_voxel")
    for r in (0.0, -1.0, np.nan, np.inf):
        _refused(call(rate=r), who, "rate")
    for t in (np.nan, np.inf, -np.inf):
        _refused(call(threshold=t), who, "threshold")
    _refused(call(x=v.ctypes.data), who, "xyz is field")
    _refused(call(vox=xyz.ctypes.data), who, "xyz is field or voxel")
    assert (xyz.view(U32) == P.XYZ_SENTINEL).all() and (voxel == P.VOXEL_SENTINEL).all() and (v == 1.0).all() and (live.value, wanted.value) == (77, 78)
    assert call() == 0 and live.value == 64 and wanted.value >= 1024  # (the same arguments, unchanged, are accepted)
    assert lib.hns_grid_birth_points(g.ptr, v.ctypes.data, None, C.byref(leafio.birth_spec(0.25, 2.5, 4, 1)), 0, None, None, 0, None, C.byref(wanted)) == 0  # a pure count


def test_object_refusals_that_need_no_device():
    g = P.host_grid("one_leaf")
    err = C.c_int(7)
    assert lib.hns_point_population_create(None, 16, C.byref(err)) is None
    _refused(err.value, "hns_point_population_create", "grid")
    err = C.c_int(7)
    assert lib.hns_point_population_create(g.ptr, 2 ** 31, C.byref(err)) is None
    _refused(err.value, "hns_point_population_create", "capacity")
    err = C.c_int(7)
    assert lib.hns_point_population_create(g.ptr, 16, C.byref(err)) is None  # a host-only grid: no device here, or no device tables there
    text = lib.hns_last_error().decode()
    if lib.hns_device_count() == 0:
        assert err.value == _lib.HNS_ERR_NO_DEVICE and "hns_point_population_create" in text and "no HIP device" in text
    else:
        _refused(err.value, "hns_point_population_create", "HNS_GRID_HOST_ONLY")
    assert lib.hns_point_population_create(None, 16, None) is None  # (err may be null)
    info, spec, n = _lib.hns_point_population_info(), leafio.birth_spec(0.0, 1.0, 1, 0), C.c_uint64(5)
    null = "null point population"
    _refused(lib.hns_point_population_set_stream(None, None), "hns_point_population_set_stream", null)
    _refused(lib.hns_point_population_set_live(None, 0), "hns_point_population_set_live", null)
    _refused(lib.hns_point_population_select(None, None, 0, 1), "hns_point_population_select", null)
    _refused(lib.hns_point_population_compact(None, None, None, 4, None), "hns_point_population_compact", null)
    _refused(lib.hns_point_population_birth(None, None, None, C.byref(spec), None, None, 0, 0), "hns_point_population_birth", null)
    _refused(lib.hns_point_population_birth_sim(None, None, b"flame", 1, C.byref(spec), None, None, 0, 0), "hns_point_population_birth_sim", null)
    _refused(lib.hns_point_population_get(None, C.byref(info)), "hns_point_population_get", null)
    _refused(lib.hns_point_population_counts(None, C.byref(n), C.byref(n)), "hns_point_population_counts", null)
    assert n.value == 5
    lib.hns_point_population_destroy(None)


def test_python_layer_argument_checks():
    g = P.host_grid("one_leaf")
    with pytest.raises(ValueError, match="negative"):
        device.PointPopulation(g, -1)
    with pytest.raises((_lib.HNSError, ValueError)) as e:  # a host-only grid has no device side
        device.PointPopulation(g, 16)
    # (without a device the refusal is HNS_ERR_NO_DEVICE, an HNSError; with one it is HNS_ERR_INVALID_ARGUMENT, which the Python layer raises as ValueError)
    assert getattr(e.value, "code", BAD) in (_lib.HNS_ERR_NO_DEVICE, BAD) and "hns_point_population_create" in str(e.value)
    with pytest.raises(ValueError, match="voxels"):
        leafio.birth_points(g, np.zeros(511, dtype=F), **P.SPEC, capacity_rows=4)
    with pytest.raises(ValueError, match="masks"):
        leafio.birth_points(g, np.zeros(512, dtype=F), np.zeros(63, dtype=np.uint8), **P.SPEC, capacity_rows=4)
    with pytest.raises(ValueError, match="xyz"):
        leafio.birth_points(g, np.zeros(512, dtype=F), **P.SPEC, capacity_rows=4, xyz=np.zeros((5, 3), dtype=F))
    with pytest.raises(_lib.HNSError, match="max_per_voxel"):
        leafio.birth_points(g, np.zeros(512, dtype=F), threshold=0.0, rate=1.0, max_per_voxel=17, seed=0, capacity_rows=4)


def test_python_constants_are_the_kernels():
    """device.POINT_POPULATION_TILE and POINT_POPULATION_SCAN_TILES, from which the GPU tests take their boundary counts, are the constants of hns_population.hip, and
    the workgroup scan is stated once, in the header both kernel files include"""
    csrc = os.path.join(ROOT, "hnanosolver_amd", "csrc")
    src = open(os.path.join(csrc, "hns_population.hip")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    assert device.POINT_POPULATION_TILE == value("kPopBlock") * value("kPopItems") == device.POINT_ORDER_TILE
    assert device.POINT_POPULATION_SCAN_TILES == value("kPopBlock") * value("kPopScanItems") == device.POINT_ORDER_SCAN_TILES
    assert re.search(r"constexpr int kPopTile = kPopBlock \* kPopItems;", src) and re.search(r"constexpr int kPopScanChunk = kPopBlock \* kPopScanItems;", src)
    stated = [f for f in sorted(os.listdir(csrc)) if re.search(r"\bunsigned block_scan\(", open(os.path.join(csrc, f)).read())]
    assert stated == ["hns_blockscan.hpp"]
    for f in ("hns_population.hip", "hns_pointorder.hip"):
        assert '#include "hns_blockscan.hpp"' in open(os.path.join(csrc, f)).read()
    assert '#include "hns_birth.hpp"' in src and '#include "hns_birth.hpp"' in open(os.path.join(csrc, "hns_leafio.cpp")).read()
    assert not re.search(r"\batomic", src.split("#include", 1)[1], flags=re.I), "hns_population.hip needs no atomic"


# mangled-name fragment: (kernel, LDS bytes its static_assert allows)
KERNELS = {
    "17k_pop_count_flags": ("k_pop_count_flags", 16),
    "17k_pop_place_slots": ("k_pop_place_slots", 16),
    "10k_pop_scan": ("k_pop_scan", 16),
    "14k_pop_set_live": ("k_pop_set_live", 0),
    "17k_pop_fill_births": ("k_pop_fill_births", 0),
    "18k_pop_count_birthsILb0": ("k_pop_count_births<false>", 16),
    "18k_pop_count_birthsILb1": ("k_pop_count_births<true>", 16),
    "18k_pop_place_birthsILb0": ("k_pop_place_births<false>", 16),
    "18k_pop_place_birthsILb1": ("k_pop_place_births<true>", 16),
    "10k_pop_rowsILb0": ("k_pop_rows<false>", 0),
    "10k_pop_rowsILb1": ("k_pop_rows<true>", 0),
}


@pytest.fixture(scope="module")
def population_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_population.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_kernel_resources(population_listing):
    """every kernel of the file is listed, nothing spills, nothing uses scratch, LDS at or below what the static_asserts state; registers printed, not gated"""
    assert len(population_listing) == len(KERNELS)
    for name, m in population_listing.items():
        found = [k for k in KERNELS if k in name]
        assert len(found) == 1, f"{name}: a kernel of hns_population.hip that is not checked here"
        kernel, lds = KERNELS[found[0]]
        print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
        assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
        assert m["group_segment_fixed_size"] <= lds, f"{kernel} uses {m['group_segment_fixed_size']} bytes of LDS, above the {lds} its static_assert states"
