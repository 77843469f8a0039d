"""Host-side mirror of the OpenVDB-free steps either side of the path (``hns_gather_leaves`` ... in include/hns.h): what
the reference's ``HNS::IndexGridBuilder`` (src/Utils/GridBuilder.hpp:87-216) and the HNanoSolver SOP's domain dilation
(src/SOP/HNanoSolver/SOP_HNanoSolver.cpp:186-199) do to OpenVDB trees, over raw 8^3 leaf buffers. PARITY UNPINNED: OpenVDB is
absent from the build image; the tests check these against brute force."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import lib

FILL_ZERO, FILL_SDF = 0, 1


def _o(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)


def gather_leaves(domain_origins, src_origins, src_values, ncomp: int = 1, fill: int = FILL_ZERO) -> np.ndarray:
    d, s = _o(domain_origins), _o(src_origins)
    v = np.ascontiguousarray(src_values, dtype=np.float32)
    assert v.size == len(s) * 512 * ncomp
    out = np.empty((len(d) * 512, ncomp) if ncomp == 3 else (len(d) * 512,), dtype=np.float32)
    _lib.check(lib.hns_gather_leaves(d.ctypes.data, len(d), s.ctypes.data, len(s), v.ctypes.data, ncomp, fill, out.ctypes.data))
    return out


def scatter_leaves(flat, n_domain: int, ncomp: int = 1):
    """-> list of per-leaf buffers (what writeIndexGrid copies into every leaf of the output grid)"""
    f = np.ascontiguousarray(flat, dtype=np.float32)
    bufs = [np.empty(512 * ncomp, dtype=np.float32) for _ in range(n_domain)]
    ptrs = (C.c_void_p * max(1, n_domain))(*[b.ctypes.data for b in bufs])
    _lib.check(lib.hns_scatter_leaves(f.ctypes.data, n_domain, ncomp, ptrs))
    return bufs


def dilate_leaves(origins, padding_voxels: int, active_masks: Optional[np.ndarray] = None) -> np.ndarray:
    o = _o(origins)
    m = None if active_masks is None else np.ascontiguousarray(active_masks, dtype=np.uint8).reshape(len(o), 64)
    n = C.c_uint64(0)
    _lib.check(lib.hns_dilate_leaves(o.ctypes.data, len(o), m.ctypes.data if m is not None else None, int(padding_voxels), None, 0, C.byref(n)))
    out = np.zeros((n.value, 3), dtype=np.int32)
    _lib.check(lib.hns_dilate_leaves(o.ctypes.data, len(o), m.ctypes.data if m is not None else None, int(padding_voxels), out.ctypes.data, n.value, C.byref(n)))
    return out


def dilate_leaf_masks(origins, padding_voxels: int, masks: Optional[np.ndarray] = None):
    """-> (origins, masks): ``dilate_leaves`` plus the dilated active masks (n x 64 uint8, byte x*8+y, bit z) that the next frame's dilation starts
    from (``hns_dilate_leaf_masks``). masks None = every voxel active."""
    o = _o(origins)
    m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8).reshape(len(o), 64)
    mp = m.ctypes.data if m is not None else None
    n = C.c_uint64(0)
    _lib.check(lib.hns_dilate_leaf_masks(o.ctypes.data, len(o), mp, int(padding_voxels), None, None, 0, C.byref(n)))
    out = np.zeros((n.value, 3), dtype=np.int32)
    out_m = np.zeros((n.value, 64), dtype=np.uint8)
    _lib.check(lib.hns_dilate_leaf_masks(o.ctypes.data, len(o), mp, int(padding_voxels), out.ctypes.data, out_m.ctypes.data, n.value, C.byref(n)))
    return out, out_m


def add_leaves(a, b, ncomp: int = 1):
    """openvdb::tools::compSum over leaf sets (``hns_add_leaves``): a, b = (origins, masks or None, values: 512 x ncomp floats per leaf) ->
    (origins, masks, values) on the union of the two leaf sets in OpenVDB leaf order; masks ORed (None = all active), values a + b where a side
    without the leaf contributes +0.0f."""
    sides = []
    for o, m, v in (a, b):
        o = _o(o)
        m = None if m is None else np.ascontiguousarray(m, dtype=np.uint8).reshape(len(o), 64)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if v.size != len(o) * 512 * ncomp:
            raise ValueError(f"add_leaves: need {len(o)} x 512 x {ncomp} floats, got {v.size}")
        sides.append((o, m, v))
    args = []
    for o, m, v in sides:
        args += [o.ctypes.data, len(o), None if m is None else m.ctypes.data, v.ctypes.data]
    n = C.c_uint64(0)
    _lib.check(lib.hns_add_leaves(*args, int(ncomp), None, None, None, 0, C.byref(n)))
    out = np.zeros((n.value, 3), dtype=np.int32)
    out_m = np.zeros((n.value, 64), dtype=np.uint8)
    out_v = np.zeros((n.value * 512, ncomp) if ncomp == 3 else (n.value * 512,), dtype=np.float32)
    _lib.check(lib.hns_add_leaves(*args, int(ncomp), out.ctypes.data, out_m.ctypes.data, out_v.ctypes.data, n.value, C.byref(n)))
    return out, out_m, out_v


def activity_fields(tolerances: dict, velocity_tolerance=None):
    """-> ctypes array of hns_activity_field: {float field name: tolerance} plus, unless velocity_tolerance is None, the velocity (name NULL)"""
    entries = [(k.encode(), 1, float(t)) for k, t in tolerances.items()]
    if velocity_tolerance is not None:
        entries.append((None, 3, float(velocity_tolerance)))
    arr = (_lib.hns_activity_field * max(1, len(entries)))()
    for i, (name, nc, tol) in enumerate(entries):
        arr[i].name, arr[i].ncomp, arr[i].tolerance = name, nc, tol
    return arr, len(entries)


def deactivate_masks(masks, fields: dict, velocity=None):
    """The host mirror of ``Sim.deactivate`` (``hns_deactivate_leaf_masks``): masks (n x 64 uint8, or None = all active), fields = {name: (values:
    512 floats per leaf, tolerance)}, velocity = (values: (n * 512, 3), tolerance) or None -> (masks, (active voxels, leaves holding one)). A voxel
    stays active iff it was active and some listed component has |x| > tolerance (NaN counts as above)."""
    vals, tols = [], {}
    for name, (v, t) in fields.items():
        vals.append(np.ascontiguousarray(v, dtype=np.float32).reshape(-1))
        tols[name] = t
    if velocity is not None:
        vals.append(np.ascontiguousarray(velocity[0], dtype=np.float32).reshape(-1))
    ncomps = [1] * len(fields) + ([3] if velocity is not None else [])
    if masks is not None:
        m = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1, 64)
        n = len(m)
    else:
        m = None
        n = vals[0].size // (512 * ncomps[0]) if vals else 0
    for v, nc in zip(vals, ncomps):
        if v.size != n * 512 * nc:
            raise ValueError(f"deactivate_masks: need {n} x 512 x {nc} floats, got {v.size}")
    arr, n_fields = activity_fields(tols, None if velocity is None else velocity[1])
    ptrs = (C.c_void_p * max(1, len(vals)))(*[v.ctypes.data for v in vals])
    out = np.zeros((n, 64), dtype=np.uint8)
    counts = (C.c_uint64 * 2)()
    _lib.check(lib.hns_deactivate_leaf_masks(n, None if m is None else m.ctypes.data, arr, ptrs, n_fields, out.ctypes.data, counts))
    return out, (int(counts[0]), int(counts[1]))


# one hns_stats record (include/hns.h), 48 bytes; records compare byte for byte through .tobytes()
STATS_DTYPE = np.dtype([("count", "<u8"), ("nan_count", "<u8"), ("min", "<f4"), ("max", "<f4"), ("max_abs", "<f4"), ("reserved", "<u4"), ("sum", "<f8"), ("sum_sq", "<f8")])
assert STATS_DTYPE.itemsize == C.sizeof(_lib.hns_stats) == 48


def leaf_stats(values, masks: Optional[np.ndarray] = None, ncomp: Optional[int] = None) -> np.ndarray:
    """The host mirror of ``Sim.stats`` and of the residual's record (``hns_leaf_stats``): values = 512 floats per leaf, or shape (n * 512, 3) (or ncomp
    = 3) for a Vec3f field; masks (n x 64 uint8) or None = every voxel -> ncomp records (STATS_DTYPE), summed in the fixed order include/hns.h states."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    nc = ncomp or (3 if (v.ndim == 2 and v.shape[1] == 3) else 1)
    if v.size % (512 * nc):
        raise ValueError(f"leaf_stats: need whole leaves of 512 x {nc} floats, got {v.size}")
    n = v.size // (512 * nc)
    m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
    if m is not None and m.size != n * 64:
        raise ValueError(f"leaf_stats: masks need {n} x 64 bytes, got {m.size}")
    out = np.zeros(nc, dtype=STATS_DTYPE)
    _lib.check(lib.hns_leaf_stats(n, None if m is None else m.ctypes.data, v.ctypes.data if n else None, nc, out.ctypes.data))
    return out


def point_leaves(xyz):
    """The seeds of a point set (``hns_point_leaves``; include/hns.h states the definition): xyz (n, 3) float32, index space -> (origins (m, 3) int32 in OpenVDB leaf
    order, masks (m, 64) uint8 with exactly the bits of the eight taps of every seeding point, the number of points that do not seed). The host mirror of
    ``device.point_leaves``."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n, skipped = C.c_uint64(0), C.c_uint64(0)
    _lib.check(lib.hns_point_leaves(p.ctypes.data, len(p), None, None, 0, C.byref(n), C.byref(skipped)))
    out = np.zeros((n.value, 3), dtype=np.int32)
    out_m = np.zeros((n.value, 64), dtype=np.uint8)
    _lib.check(lib.hns_point_leaves(p.ctypes.data, len(p), out.ctypes.data, out_m.ctypes.data, n.value, C.byref(n), C.byref(skipped)))
    return out, out_m, int(skipped.value)


LEVELS = {"leaf": 0, "voxel": 1}  # what a point order sorts by (include/hns.h: "Level")


def sort_level(level) -> int:
    """"leaf" / "voxel" (or the ABI's 0 / 1) -> the ABI's level"""
    if level in LEVELS:
        return LEVELS[level]
    if isinstance(level, (int, np.integer)) and not isinstance(level, bool) and int(level) in (0, 1):
        return int(level)
    raise ValueError(f'level must be "leaf" or "voxel" (0 or 1), got {level!r}')


def sort_points(grid, xyz, level="voxel"):
    """The leaf order of a point set (``hns_grid_sort_points``; include/hns.h states the definition): xyz (n, 3) float32, index space, on `grid` (a host-only grid will do)
    -> (perm (n,) uint32: the stable order by voxel key, or by leaf with level="leaf"; keys (n,) uint32: the key of point perm[r]; leaf_start (leaves + 3,) uint32: the
    ranks each leaf owns, then the outside points, then the points that do not sort, then n). The host mirror of ``device.PointOrder.sort``."""
    lv = sort_level(level)
    p = np.ascontiguousarray(xyz, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("sort_points: xyz must be an (n, 3) array")
    n = len(p)
    perm, keys = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    leaf_start = np.zeros(grid.leaf_count() + 3, dtype=np.uint32)
    _lib.check(lib.hns_grid_sort_points(grid.ptr, p.ctypes.data if n else None, n, lv, perm.ctypes.data, keys.ctypes.data, leaf_start.ctypes.data))
    return perm, keys, leaf_start


def point_neighbours(grid, xyz, radius):
    """Point neighbourhoods (``hns_grid_point_neighbours``; include/hns.h states the definition): xyz (n, 3) float32, index space, on `grid` (a host-only grid will do),
    0 < radius <= 2 -> (count (n,) uint32: the points around each point; density (n,) float32: the sum of their weights; push (n, 3) float32: the weighted sum of the unit
    vectors away from them), rows in the order of xyz. The host mirror of ``device.PointOrder.neighbours``."""
    p = np.ascontiguousarray(xyz, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("point_neighbours: xyz must be an (n, 3) array")
    n = len(p)
    count, density, push = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    _lib.check(lib.hns_grid_point_neighbours(grid.ptr, p.ctypes.data if n else None, n, float(radius), count.ctypes.data, density.ctypes.data, push.ctypes.data))
    return count, density, push


def birth_spec(threshold, rate, max_per_voxel, seed, fill=True) -> _lib.hns_birth_spec:
    """the ABI's hns_birth_spec (include/hns.h: "BIRTH AND DEATH OF POINTS"); the library refuses what is outside the rule"""
    return _lib.hns_birth_spec(float(threshold), float(rate), int(max_per_voxel), int(seed) & 0xFFFFFFFF, int(bool(fill)))


def birth_points(grid, field, masks=None, *, threshold, rate, max_per_voxel, seed, fill=True, start=0, capacity_rows, xyz=None, voxel=None):
    """Points born from a field (``hns_grid_birth_points``; include/hns.h states the rule): field (voxels,) float32 on `grid` (a host-only grid will do), masks None or
    (leaves, 64) uint8. Every eligible voxel bears 0 .. max_per_voxel points, in voxel order, into rows start .. of xyz ((capacity_rows, 3) float32) and voxel
    ((capacity_rows,) uint32), made here (zeroed) when None -> (xyz, voxel, live, wanted): wanted = start + the births, live = min(wanted, capacity_rows); with fill the
    rows live .. capacity_rows - 1 are NaN / 0xFFFFFFFF. The host mirror of ``device.PointPopulation.birth``."""
    f = np.ascontiguousarray(field, dtype=np.float32).reshape(-1)
    if f.size != grid.leaf_count() * 512:
        raise ValueError(f"birth_points: the field has {f.size} values, the grid {grid.leaf_count() * 512} voxels")
    m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
    if m is not None and m.size != grid.leaf_count() * 64:
        raise ValueError(f"birth_points: masks need {grid.leaf_count()} x 64 bytes, got {m.size}")
    rows = int(capacity_rows)
    xyz = np.zeros((rows, 3), dtype=np.float32) if xyz is None else xyz
    voxel = np.zeros(rows, dtype=np.uint32) if voxel is None else voxel
    for name, a, shape, dt in (("xyz", xyz, (rows, 3), np.float32), ("voxel", voxel, (rows,), np.uint32)):
        if a.dtype != dt or tuple(a.shape) != shape or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"birth_points: {name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
    spec = birth_spec(threshold, rate, max_per_voxel, seed, fill)
    live, wanted = C.c_uint64(0), C.c_uint64(0)
    _lib.check(lib.hns_grid_birth_points(grid.ptr, f.ctypes.data, None if m is None else m.ctypes.data, C.byref(spec), int(start), xyz.ctypes.data if rows else None,
                                         voxel.ctypes.data if rows else None, rows, C.byref(live), C.byref(wanted)))
    return xyz, voxel, int(live.value), int(wanted.value)


def union_leaves(a, b) -> np.ndarray:
    a, b = _o(a), _o(b)
    n = C.c_uint64(0)
    _lib.check(lib.hns_union_leaves(a.ctypes.data, len(a), b.ctypes.data, len(b), None, 0, C.byref(n)))
    out = np.zeros((n.value, 3), dtype=np.int32)
    _lib.check(lib.hns_union_leaves(a.ctypes.data, len(a), b.ctypes.data, len(b), out.ctypes.data, n.value, C.byref(n)))
    return out
