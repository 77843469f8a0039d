"""Kernel-level calls of libhns.so on device-resident torch tensors.

PyTorch is plumbing here: it owns device memory and streams; every computation is a HIP kernel of libhns.so reached
through the C ABI (``hns_dev_*`` / ``hns_sim_*`` in include/hns.h). Velocity tensors are ``(N, 3)`` float32 (Vec3f AoS, the
host layout). There is no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, leafio
from ._lib import hns_combustion_params, hns_field, lib
from .api import CombustionParams, IndexGridHandle, _raise, create_grid_from_leaves, splat_spec, stored_splat_spec  # noqa: F401


def _torch():
    import torch

    return torch


def _ptr(t) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise RuntimeError("hnanosolver_amd.device: tensor is not on a HIP device (there is no CPU fallback)")
    if t.dtype != _torch().float32 and t.dtype != _torch().int32:
        raise TypeError("expected float32 / int32 tensor")
    if not t.is_contiguous():
        raise TypeError("expected a contiguous tensor")
    return t.data_ptr()


def current_stream() -> int:
    return int(_torch().cuda.current_stream().cuda_stream)


def _stream(stream: Optional[int]) -> int:
    """a hipStream_t as an integer; None: torch's current stream"""
    return current_stream() if stream is None else int(stream)


def _ptrs(tensors):
    """the device addresses of `tensors` as a void* array (one entry at the least: there is no empty ctypes array to pass)"""
    p = [_ptr(t) for t in tensors]
    return (C.c_void_p * max(1, len(p)))(*p)


def _names(names):
    """`names` as a char* array, likewise"""
    b = [n.encode() for n in names]
    return (C.c_char_p * max(1, len(b)))(*b)


def _xyz3(what: str, xyz, shape: str = "an (n, 3)") -> None:
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != _torch().float32:
        raise ValueError(f"{what}: xyz must be {shape} float32 tensor")


class _Handle:
    """An object of libhns.so behind ``_ptr``: made by a create call whose last argument is the status, gone with ``close`` -- at the end of a ``with`` block and with the
    Python object too. _destroy: the name of the library's destroy function. _sim, _made_by: the Sim whose grid the object was made on and the method that made it."""

    _destroy = ""
    _ptr = 0
    _sim = None
    _made_by = ""

    def _create(self, create, *args) -> None:
        err = C.c_int(0)
        self._ptr = create(*args, C.byref(err))
        if not self._ptr:
            _raise(err.value if err.value < 0 else _lib.HNS_ERR_RUNTIME)

    def _live(self) -> int:
        name = type(self).__name__
        if not self._ptr:
            raise RuntimeError(f"{name}: the object is closed")
        if self._sim is not None and self._sim.grid is not self.grid:
            raise RuntimeError(f"{name}: the sim has moved onto another grid (regrid) since {self._made_by} made this object; make a new one on the sim's current grid")
        return self._ptr

    def close(self) -> None:
        if self._ptr:
            getattr(lib, self._destroy)(self._ptr)
            self._ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _row_move(what: str, n: int, ran: str, src, dst):
    """The checks of a move of the first `n` rows of src into dst (made here when None) behind the object's last `ran` -> (dst, bytes of a row)"""
    for name, t in (("src", src), ("dst", dst)):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dim() < 1):
            raise TypeError(f"{what}: {name} must be a contiguous tensor of at least one dimension on a HIP device")
    row_bytes = src.element_size() * int(np.prod(src.shape[1:], dtype=np.int64))
    if row_bytes % 4 or not 4 <= row_bytes <= 64:
        raise ValueError(f"{what}: a row of src has {row_bytes} bytes (a multiple of 4 in 4 .. 64)")
    if dst is None:
        dst = _torch().empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if dst.dtype != src.dtype or tuple(dst.shape[1:]) != tuple(src.shape[1:]):
        raise ValueError(f"{what}: dst rows are not src rows ({tuple(dst.shape[1:])} {dst.dtype} against {tuple(src.shape[1:])} {src.dtype})")
    if src.shape[0] < n or dst.shape[0] < n:
        raise ValueError(f"{what}: src has {src.shape[0]} rows and dst {dst.shape[0]}, the last {ran} {n}")
    return dst, row_bytes


def advect_vector(grid: IndexGridHandle, u, out, dt: float, inv_dx: float, sdf=None, has_collision: bool = False):
    _raise(lib.hns_dev_advect_vector(grid.ptr, _ptr(u), _ptr(out), _ptr(sdf), int(has_collision), dt, inv_dx, current_stream()))
    return out


def advect_scalar(grid: IndexGridHandle, u, src, dst, dt: float, inv_dx: float, sdf=None, has_collision: bool = False):
    _raise(lib.hns_dev_advect_scalar(grid.ptr, _ptr(u), _ptr(src), _ptr(dst), _ptr(sdf), int(has_collision), dt, inv_dx, current_stream()))
    return dst


def _advect_many(call, grid, u, srcs, dsts, dt, inv_dx, sdf, has_collision):
    _raise(call(grid.ptr, _ptr(u), _ptrs(srcs), _ptrs(dsts), len(srcs), _ptr(sdf), int(has_collision), dt, inv_dx, current_stream()))
    return dsts


def advect_scalars(grid: IndexGridHandle, u, srcs: Sequence, dsts: Sequence, dt: float, inv_dx: float, sdf=None, has_collision: bool = False):
    return _advect_many(lib.hns_dev_advect_scalars, grid, u, srcs, dsts, dt, inv_dx, sdf, has_collision)


def advect_scalar_multi(grid: IndexGridHandle, u, srcs: Sequence, dsts: Sequence, dt: float, inv_dx: float, sdf=None, has_collision: bool = False):
    """advect_scalar of every field of `srcs` with one back-trace (``hns_dev_advect_scalar_multi``): dsts[i] is bit-identical to ``advect_scalar`` of srcs[i]."""
    return _advect_many(lib.hns_dev_advect_scalar_multi, grid, u, srcs, dsts, dt, inv_dx, sdf, has_collision)


def advect_scalars_ahead(grid: IndexGridHandle, u, srcs: Sequence, dsts: Sequence, adv_out, dt: float, inv_dx: float):
    """advect_scalars over `srcs` and advect_vector(u) into `adv_out`, one launch (``hns_dev_advect_scalars_ahead``)."""
    _raise(lib.hns_dev_advect_scalars_ahead(grid.ptr, _ptr(u), _ptrs(srcs), _ptrs(dsts), len(srcs), _ptr(adv_out), dt, inv_dx, current_stream()))
    return dsts, adv_out


def divergence(grid: IndexGridHandle, u, div, inv_dx: float):
    _raise(lib.hns_dev_divergence(grid.ptr, _ptr(u), _ptr(div), inv_dx, current_stream()))
    return div


def rbgs_color(grid: IndexGridHandle, div, p, dx: float, omega: float, color: int):
    _raise(lib.hns_dev_rbgs_color(grid.ptr, _ptr(div), _ptr(p), dx, omega, color, current_stream()))
    return p


def rbgs_iterate(grid: IndexGridHandle, div, p_a, p_b, dx: float, omega: float, iterations: int):
    """Returns the tensor (p_a or p_b) that holds the result."""
    in_b = C.c_int(0)
    _raise(lib.hns_dev_rbgs_iterate(grid.ptr, _ptr(div), _ptr(p_a), _ptr(p_b), dx, omega, iterations, C.byref(in_b), current_stream()))
    return p_b if in_b.value else p_a


def rbgs_plan(grid: IndexGridHandle, iterations: int):
    """(description of the SOR kernel form this grid is swept with, kernel launches for `iterations`, iterations per launch)"""
    buf = C.create_string_buffer(256)
    n, k = C.c_int(0), C.c_int(0)
    _raise(lib.hns_grid_rbgs_plan(grid.ptr, iterations, buf, 256, C.byref(n), C.byref(k)))
    return buf.value.decode(), n.value, k.value


def time_rbgs(grid: IndexGridHandle, div, p_a, p_b, dx: float, omega: float, iterations: int, reps: int) -> float:
    """Mean milliseconds per fused-iteration launch, measured with hipEvents on the launch stream."""
    ms = C.c_float(0.0)
    _raise(lib.hns_dev_time_rbgs(grid.ptr, _ptr(div), _ptr(p_a), _ptr(p_b), dx, omega, iterations, reps, C.byref(ms), current_stream()))
    return float(ms.value)


def subtract_pressure_gradient(grid: IndexGridHandle, u, p, out, inv_dx: float, sdf=None, has_collision: bool = False):
    _raise(lib.hns_dev_subtract_pressure_gradient(grid.ptr, _ptr(u), _ptr(p), _ptr(out), _ptr(sdf), int(has_collision), inv_dx, current_stream()))
    return out


def combustion_oxygen(fuel, waste, temperature, div, flame, out_fuel, out_waste, out_temperature, out_flame, temp_gain: float, expansion: float):
    _raise(lib.hns_dev_combustion_oxygen(_ptr(fuel), _ptr(waste), _ptr(temperature), _ptr(div), _ptr(flame), _ptr(out_fuel), _ptr(out_waste),
                                         _ptr(out_temperature), _ptr(out_flame), temp_gain, expansion, fuel.numel(), current_stream()))


def temperature_buoyancy(u, temperature, out, dt: float, ambient: float, strength: float):
    _raise(lib.hns_dev_temperature_buoyancy(_ptr(u), _ptr(temperature), _ptr(out), dt, ambient, strength, temperature.numel(), current_stream()))
    return out


def vorticity_confinement(grid: IndexGridHandle, u, out, dt: float, inv_dx: float, scale: float, factor_scale: float):
    _raise(lib.hns_dev_vorticity_confinement(grid.ptr, _ptr(u), _ptr(out), dt, inv_dx, scale, factor_scale, current_stream()))
    return out


def enforce_collision_boundaries(grid: IndexGridHandle, u, sdf, voxel_size: float):
    _raise(lib.hns_dev_enforce_collision_boundaries(grid.ptr, _ptr(u), _ptr(sdf), voxel_size, current_stream()))
    return u


def pack_leaves(field, leaf_ids, packed, ncomp: int = 1):
    _raise(lib.hns_dev_pack_leaves(_ptr(field), _ptr(leaf_ids), leaf_ids.numel(), _ptr(packed), ncomp, current_stream()))
    return packed


def unpack_leaves(packed, leaf_ids, field, ncomp: int = 1):
    _raise(lib.hns_dev_unpack_leaves(_ptr(packed), _ptr(leaf_ids), leaf_ids.numel(), _ptr(field), ncomp, current_stream()))
    return field


def _byte_ptr(t) -> int:
    if t is None:
        return 0
    if not t.is_cuda or t.dtype != _torch().uint8 or not t.is_contiguous():
        raise TypeError("expected a contiguous uint8 tensor on a HIP device")
    return t.data_ptr()


def _ncomp(t) -> int:
    return 3 if (t.dim() == 2 and t.shape[1] == 3) else 1


def sample_points(grid: IndexGridHandle, fields: Sequence, xyz, outs: Optional[Sequence] = None):
    """Every field of `fields` -- (N,) float tensors and (N, 3) Vec3f tensors in any mix -- at the positions xyz, an (n, 3) float32 tensor in INDEX space
    (``hns_dev_sample_points``): the advection kernels' trilinear samplers, 0 outside the domain. outs[i] is (n,) or (n, 3) like its field, made here when
    outs is None; up to eight fields share a launch, and outs[i] is bit-identical to a call with fields[i] alone. Asynchronous on the current stream."""
    n, k = xyz.shape[0], len(fields)
    nc = [_ncomp(f) for f in fields]
    if outs is None:
        outs = [_torch().empty((n, 3) if c == 3 else (n,), dtype=_torch().float32, device=xyz.device) for c in nc]
    _raise(lib.hns_dev_sample_points(grid.ptr, _ptrs(fields), (C.c_int * max(1, k))(*nc), k, _ptr(xyz), n, _ptrs(outs), current_stream()))
    return outs


def trace_points(grid: IndexGridHandle, vel, xyz, dt: float, inv_dx: float, order: int = 2, steps: int = 1, status=None):
    """`steps` steps of the points xyz ((n, 3) float32, index space, moved IN PLACE) through the velocity `vel` (``hns_dev_trace_points``): order 1 Euler, 2 midpoint,
    4 Runge-Kutta; a negative dt traces back. status: None or a uint8 tensor of n bytes, 1 where the final position is finite and inside a leaf. Asynchronous on
    the current stream."""
    _raise(lib.hns_dev_trace_points(grid.ptr, _ptr(vel), _ptr(xyz), xyz.shape[0], dt, inv_dx, int(order), int(steps), _byte_ptr(status), current_stream()))
    return xyz


COLLIDE_MODES = {"stop": _lib.HNS_COLLIDE_STOP, "push": _lib.HNS_COLLIDE_PUSH, "kill": _lib.HNS_COLLIDE_KILL}


def _collision(who: str, mode, threshold: float, skin: float, iterations: int):
    if mode not in COLLIDE_MODES:
        raise ValueError(f"{who}: mode must be one of {sorted(COLLIDE_MODES)}, not {mode!r}")
    return _lib.hns_point_collision(COLLIDE_MODES[mode], float(threshold), float(skin), int(iterations))


def trace_points_collide(grid: IndexGridHandle, vel, sdf, xyz, dt: float, inv_dx: float, order: int = 2, steps: int = 1, *, mode: str, threshold: float = 0.0,
                         skin: float = 1 / 16, iterations: int = 2, status=None, hit=None):
    """``trace_points`` against the collision SDF `sdf` (a float field of the grid), tested after every step inside the launch (``hns_dev_trace_points_collide``). A point
    whose step ends where the SDF's sample is below `threshold` is, by `mode`, put back ("stop"), pushed out along the SDF's normal by its depth plus `skin` voxels, up to
    `iterations` times, and put back if still inside ("push"), or frozen and marked dead ("kill"). status: None or a uint8 tensor of n bytes, 1 where the point is alive,
    finite and inside a leaf. hit: None or a uint8 tensor of n bytes: 1 pushed, 2 put back, 4 killed, 8 started inside, ORed. Asynchronous on the current stream."""
    spec = _collision("trace_points_collide", mode, threshold, skin, iterations)
    _raise(lib.hns_dev_trace_points_collide(grid.ptr, _ptr(vel), _ptr(sdf), _ptr(xyz), xyz.shape[0], dt, inv_dx, int(order), int(steps), C.byref(spec), _byte_ptr(status),
                                            _byte_ptr(hit), current_stream()))
    return xyz


def _u64_ptr(t) -> int:
    if t is None:
        return 0
    if not t.is_cuda or t.dtype != _torch().int64 or not t.is_contiguous() or t.numel() < 1:
        raise TypeError("expected a contiguous int64 tensor of one element on a HIP device")
    return t.data_ptr()


def _radius_ptr(t, n) -> int:
    if not t.is_cuda or t.dtype != _torch().float32 or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise TypeError("radius: expected a number or a contiguous float32 tensor of one radius per point on a HIP device")
    return t.data_ptr()


def splat_points(grid: IndexGridHandle, fields: Sequence, xyz, values: Sequence, log2_quantum: int = -32, status=None, rejected=None, *, kernel: str = "trilinear",
                 mode: str = "add", radius=None, max_radius: Optional[float] = None, min_weight: float = 0.0):
    """The transpose of ``sample_points`` (``hns_dev_splat_points``): every point adds weight * value to the eight voxels of its cell, IN PLACE into `fields` -- up to
    eight (N,) float and (N, 3) Vec3f tensors in any mix -- from values[i], (n,) or (n, 3) like its field, at the positions xyz ((n, 3) float32, index space). Terms are
    rounded once to multiples of 2^log2_quantum and summed as 64-bit integers, so the result does not depend on the order the atomics retire in and equals
    ``api.splat_points_host`` in every byte. status: None or a uint8 tensor of n bytes, the taps of each point that landed in a leaf (0 .. 8); rejected: None or an int64
    tensor of one element the call adds the number of landed but unaccepted terms to (NaN, inf, beyond 2^62 quanta). Asynchronous on the current stream.
    kernel="radial": every point rasterises the footprint of `radius` voxels (0 < radius <= 4; a number, or a float32 device tensor of one radius per point with its
    upper bound in `max_radius`) with the weights (1 - d^2/r^2)^2 (``hns_splat_spec`` in include/hns.h), and status is 2 (the whole footprint landed), 1 (a part) or 0.
    mode="average": the fields are REPLACED by the weighted mean sum(w v) / max(sum(w), min_weight) wherever a weight arrived. The spec is stored with the grid for the call
    and the previous one put back; a radius tensor must stay alive until the call has run."""
    spec = splat_spec(kernel, mode, radius, max_radius, min_weight, pointer=lambda t: _radius_ptr(t, xyz.shape[0]))
    k = len(fields)
    with stored_splat_spec(lib.hns_grid_set_splat_spec, lib.hns_grid_get_splat_spec, grid.ptr, spec):
        _raise(lib.hns_dev_splat_points(grid.ptr, _ptrs(fields), (C.c_int * max(1, k))(*[_ncomp(f) for f in fields]), k, _ptr(xyz), _ptrs(values), xyz.shape[0], int(log2_quantum),
                                        _byte_ptr(status), _u64_ptr(rejected), current_stream()))
    return fields


def point_leaves(xyz):
    """The seeds of the points xyz, an (n, 3) float32 device tensor in index space (``hns_dev_point_leaves``): the leaves under the eight taps of every point's cell and,
    per leaf, exactly the tap bits -> (origins (m, 3) int32 in OpenVDB leaf order, masks (m, 64) uint8, the number of points that do not seed), numpy arrays equal in
    every byte to ``leafio.point_leaves``. With ``create_grid_from_leaves`` the origins are a fresh grid around a particle set. Synchronous on the current stream."""
    n = int(xyz.shape[0])
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("point_leaves: xyz must be an (n, 3) tensor")
    ptr, dev, st = (_ptr(xyz) if n else 0), (xyz.device.index or 0), current_stream()
    m, skipped = C.c_uint64(0), C.c_uint64(0)
    cap = min(8 * n, 1 << 16)  # a guess that spares most point sets the second call: a call runs the kernels whether or not its arrays are large enough
    while True:
        out = np.zeros((cap, 3), dtype=np.int32)
        out_m = np.zeros((cap, 64), dtype=np.uint8)
        _raise(lib.hns_dev_point_leaves(dev, ptr, n, out.ctypes.data, out_m.ctypes.data, cap, C.byref(m), C.byref(skipped), st))
        if m.value <= cap:
            return np.ascontiguousarray(out[: m.value]), np.ascontiguousarray(out_m[: m.value]), int(skipped.value)
        cap = int(m.value)


POINT_ORDER_TILE = 2048        # points of one tile of the radix sort (hns_pointorder.hip: kOrderTile)
POINT_ORDER_SCAN_TILES = 1024  # tiles one round of a scan workgroup covers (kScanChunk): beyond POINT_ORDER_TILE * POINT_ORDER_SCAN_TILES points the scan carries
SPLAT_ROWS = {"original": 0, "ranked": 1}  # the per-point arrays of an ordered splat: those the sort saw, or their gather (include/hns.h: hns_point_order_splat)


class _DeviceWords:
    """`n` 32-bit words of device memory at `ptr` for ``torch.as_tensor``: a view, no copy; `owner` is kept alive with it. shape, typestr: another shape and element
    type ("<f4", "|u1") over the same memory"""

    def __init__(self, ptr: int, n: int, owner, shape=None, typestr: str = "<i4"):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape) if shape is not None else (int(n),), "typestr": typestr, "data": (int(ptr), False), "strides": None,
                                         "version": 2}


class PointOrder(_Handle):
    """The leaf order of a point set on the device (``hns_point_order``; include/hns.h states the definition): a stable sort of up to `capacity` points by the voxel -- or
    the leaf -- of their cell on `grid`, the per-leaf ranges, and the moves that carry per-point rows through the permutation and back. The point kernels run some five
    times faster on points in this order. Buffers come from the pool of device memory once, here; ``sort``, ``gather`` and ``scatter`` allocate nothing in the library
    and are asynchronous on the stream of the last ``sort``. Holds the grid handle: the grid outlives the object."""

    _destroy, _made_by = "hns_point_order_destroy", "Sim.point_order"

    def __init__(self, grid: IndexGridHandle, capacity: int, _sim=None):
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"PointOrder: capacity {capacity} is negative")
        self.grid, self.capacity, self._sim = grid, capacity, _sim
        self._create(lib.hns_point_order_create, grid.ptr, capacity)
        self.n, self.level = 0, None

    def sort(self, xyz, level="voxel", stream: Optional[int] = None):
        """Sort the points xyz ((n, 3) float32 device tensor, index space, only read; n <= capacity) by "voxel" or by "leaf". stream: a hipStream_t as an integer, None = torch's
        current stream; this call and every later ``gather`` / ``scatter`` are ordered on it and on nothing else. Returns self; ``perm``, ``keys`` and
        ``leaf_start`` are the results."""
        ptr, lv = self._live(), leafio.sort_level(level)
        _xyz3("PointOrder.sort", xyz)
        n = int(xyz.shape[0])
        if n > self.capacity:
            raise ValueError(f"PointOrder.sort: {n} points are above the capacity {self.capacity}")
        _raise(lib.hns_point_order_set_stream(ptr, _stream(stream)))
        _raise(lib.hns_point_order_sort(ptr, _ptr(xyz) if n else 0, n, lv))
        self.n, self.level = n, ("voxel" if lv else "leaf")
        return self

    def _info(self):
        info = _lib.hns_point_order_info()
        _raise(lib.hns_point_order_get(self._live(), C.byref(info)))
        return info

    def _words(self, ptr, n):
        if n == 0:
            return _torch().empty(0, dtype=_torch().int32, device="cuda")
        return _torch().as_tensor(_DeviceWords(ptr, n, self), device="cuda")

    @property
    def perm(self):
        """perm[r]: the index in xyz of the point of rank r -- an int32 view of the object's buffer (n entries), valid until the next sort; no wait"""
        info = self._info()
        return self._words(info.perm, info.n)

    @property
    def keys(self):
        """keys[r]: the key of point perm[r] at the sort's level -- a view of the uint32 words as int32, valid until the next sort; no wait"""
        info = self._info()
        return self._words(info.keys, info.n)

    @property
    def leaf_start(self):
        """leaves + 3 entries: leaf q owns ranks leaf_start[q] .. leaf_start[q + 1]; [leaves] starts the outside points, [leaves + 1] the points that do not sort,
        [leaves + 2] = n -- an int32 view, valid until the next sort; no wait"""
        info = self._info()
        return self._words(info.leaf_start, info.n_leaves + 3)

    def _move(self, call, what, src, dst):
        ptr = self._live()
        if self.level is None:
            raise RuntimeError(f"PointOrder.{what}: no sort has run on this object")
        dst, row_bytes = _row_move(f"PointOrder.{what}", self.n, "sort", src, dst)
        if self.n:
            _raise(call(ptr, src.data_ptr(), dst.data_ptr(), row_bytes))
        return dst

    def gather(self, src, dst=None):
        """dst row r = src row perm[r] for the n rows of the last sort -> dst (made here when None; rows of a longer dst beyond n keep their bytes). Rows are
        src.shape[1:], 4 .. 64 bytes in whole 32-bit words. On the stream of the last sort."""
        return self._move(lib.hns_point_order_gather, "gather", src, dst)

    def scatter(self, src, dst=None):
        """dst row perm[r] = src row r: the way back, ``scatter(gather(x)) == x``"""
        return self._move(lib.hns_point_order_scatter, "scatter", src, dst)

    def _splat_rows(self, what, rows, xyz, per_point) -> int:
        """the ABI's `rows` of an ordered splat, after the checks that need no device: a sort has run, and every per-point array has the n rows of that sort"""
        if rows not in SPLAT_ROWS:
            raise ValueError(f'{what}: rows must be "original" (the arrays the sort saw) or "ranked" (their gather), got {rows!r}')
        if self.level is None:
            raise RuntimeError(f"{what}: no sort has run on this object")
        _xyz3(what, xyz)
        for name, t in [("xyz", xyz), *per_point]:
            if t is not None and t.shape[0] != self.n:
                raise ValueError(f"{what}: {name} has {t.shape[0]} rows, the last sort {self.n}")
        return SPLAT_ROWS[rows]

    def splat(self, fields: Sequence, xyz, values: Sequence, log2_quantum: int = -32, status=None, rejected=None, *, rows: str = "original", kernel: str = "trilinear",
              mode: str = "add", radius=None, max_radius: Optional[float] = None, min_weight: float = 0.0):
        """``splat_points`` for the points of the last sort, through the order (``hns_point_order_splat``): each leaf's voxels are summed on chip by one workgroup and the
        fields written with plain stores. The same bytes, status and rejected count as ``splat_points(self.grid, ...)`` of the same points. rows="original": xyz,
        values, status and a radius tensor are the arrays the sort saw; rows="ranked": they are in sorted order (``gather``). xyz must hold the positions of the last
        sort. Asynchronous on the stream of the last sort. A point set concentrated in a few leaves is summed by a few workgroups: ``splat_points`` is then faster."""
        r = self._splat_rows("PointOrder.splat", rows, xyz, [(f"values[{i}]", v) for i, v in enumerate(values)] + [("status", status)])
        ptr = self._live()
        spec = splat_spec(kernel, mode, radius, max_radius, min_weight, pointer=lambda t: _radius_ptr(t, self.n))
        k = len(fields)
        with stored_splat_spec(lib.hns_grid_set_splat_spec, lib.hns_grid_get_splat_spec, self.grid.ptr, spec):
            _raise(lib.hns_point_order_splat(ptr, _ptrs(fields), (C.c_int * max(1, k))(*[_ncomp(f) for f in fields]), k, _ptr(xyz) if self.n else 0, _ptrs(values), r, int(log2_quantum),
                                             _byte_ptr(status), _u64_ptr(rejected)))
        return fields

    @property
    def cell_start(self):
        """512 * leaves + 1 entries: voxel v owns ranks cell_start[v] .. cell_start[v + 1] of the last sort, which must be by "voxel" (``hns_point_order_cells``) -- an
        int32 view of the object's table, built on the stream of the last sort by the first call behind it, valid until the next sort; no wait"""
        if self.level is None:
            raise RuntimeError("PointOrder.cell_start: no sort has run on this object")
        table = C.c_void_p(0)
        _raise(lib.hns_point_order_cells(self._live(), C.byref(table)))
        return self._words(table.value, 512 * self.grid.leaf_count() + 1)

    def neighbours(self, xyz, radius: float, *, rows: str = "original", count=True, density=True, push=True):
        """The points around each point of the last sort, which must be by "voxel" (``hns_point_order_neighbours``; include/hns.h states the definition): within `radius`
        (0 < radius <= 2 voxels) of every point the number of other points, the sum of their weights (1 - d^2 / radius^2)^2 and the weighted sum of the unit vectors away
        from them, each sum exact in multiples of 2^-32: the bytes of ``leafio.point_neighbours``. rows="original": xyz and the outputs are in the order the sort saw;
        rows="ranked": in sorted order (``gather``). xyz must hold the positions of the last sort. count, density, push: True (made here), False (left out) or a tensor to
        write -- (n,) int32 holding the uint32 words, (n,) float32, (n, 3) float32. -> a dict of the outputs asked for. Asynchronous on the stream of the last sort."""
        r = self._splat_rows("PointOrder.neighbours", rows, xyz, [])
        ptr, torch = self._live(), _torch()
        out = {}
        for name, want, shape, dtype in (("count", count, (self.n,), torch.int32), ("density", density, (self.n,), torch.float32), ("push", push, (self.n, 3), torch.float32)):
            if want is False or want is None:
                continue
            t = torch.empty(shape, dtype=dtype, device=xyz.device) if want is True else want
            if not t.is_cuda or not t.is_contiguous() or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError(f"PointOrder.neighbours: {name} must be a contiguous {dtype} tensor of shape {shape} on a HIP device")
            out[name] = t
        if not out:
            raise ValueError("PointOrder.neighbours: none of count, density and push is asked for")
        addr = lambda name: out[name].data_ptr() if name in out else 0
        if self.n:  # (the outputs of no points are empty tensors, which have no address)
            _raise(lib.hns_point_order_neighbours(ptr, _ptr(xyz), r, float(radius), addr("count"), addr("density"), addr("push")))
        return out


POINT_POPULATION_TILE = 2048        # items -- points of a select, voxels of a birth -- of one tile (hns_population.hip: kPopTile)
POINT_POPULATION_SCAN_TILES = 1024  # tiles one round of the scan workgroup covers (kPopScanChunk): beyond POINT_POPULATION_TILE * POINT_POPULATION_SCAN_TILES items the scan carries


class PointPopulation(_Handle):
    """Birth and death of points on the device (``hns_point_population``; include/hns.h states the rules): ``select`` turns a flag byte per point into a slot per kept
    point, ``compact`` moves the rows of any attribute array through the slots, ``birth`` makes points from a field -- 0 .. max_per_voxel per voxel --, and the live count
    stays on the device: nothing here waits for the host but ``counts``. A frame loop keeps calling every point kernel with n = capacity; the rows beyond the live count
    hold NaN positions, which those kernels treat as nothing. Buffers come from the pool of device memory once, here. ``select``, ``birth`` and ``set_live`` bind the
    stream they are given (None: torch's current stream); ``compact`` runs on the stream bound last. Holds the grid handle: the grid outlives the object."""

    _destroy, _made_by = "hns_point_population_destroy", "Sim.point_population"

    def __init__(self, grid: IndexGridHandle, capacity: int, _sim=None):
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"PointPopulation: capacity {capacity} is negative")
        self.grid, self.capacity, self._sim = grid, capacity, _sim
        self._create(lib.hns_point_population_create, grid.ptr, capacity)
        self.n = None  # of the last select

    def _bind(self, stream) -> int:
        ptr = self._live()
        _raise(lib.hns_point_population_set_stream(ptr, _stream(stream)))
        return ptr

    def set_live(self, n: int, stream: Optional[int] = None):
        """live = wanted = n, on the stream: for a caller that already holds n rows"""
        _raise(lib.hns_point_population_set_live(self._bind(stream), int(n)))
        return self

    def select(self, flags, at_least: int = 1, stream: Optional[int] = None):
        """Point i of the n = len(flags) points (a uint8 device tensor, only read; n <= capacity) is kept iff flags[i] >= at_least: the status of ``trace_points`` or of a
        splat is such a flag. Afterwards ``slot`` holds, per point, its row among the kept ones or -1, and live = the number kept. Returns self."""
        n = int(flags.shape[0])
        if flags.dim() != 1:
            raise ValueError("PointPopulation.select: flags must be a one-dimensional uint8 tensor")
        if n > self.capacity:
            raise ValueError(f"PointPopulation.select: {n} points are above the capacity {self.capacity}")
        _raise(lib.hns_point_population_select(self._bind(stream), _byte_ptr(flags) if n else 0, n, int(at_least)))
        self.n = n
        return self

    @property
    def slot(self):
        """slot[i]: the row of point i among the kept ones, -1 for a dropped point -- an int32 view of the object's buffer (the n of the last select), valid until the
        next select; no wait"""
        info = _lib.hns_point_population_info()
        _raise(lib.hns_point_population_get(self._live(), C.byref(info)))
        if info.n == 0:
            return _torch().empty(0, dtype=_torch().int32, device="cuda")
        return _torch().as_tensor(_DeviceWords(info.slot, info.n, self), device="cuda")

    def compact(self, src, dst=None, fill=None):
        """dst row slot[i] = src row i for every point the last select kept -> dst (made here, n rows, when None). Rows are src.shape[1:], 4 .. 64 bytes in whole 32-bit
        words. fill: None -- the rows of dst from the live count on keep their bytes --, or a float (its float32 bits) or an int (a 32-bit word) that every word of the rows
        live .. n - 1 becomes: ``fill=float("nan")`` for positions. Rows of a longer dst beyond n are never touched. On the stream bound last."""
        ptr = self._live()
        if self.n is None:
            raise RuntimeError("PointPopulation.compact: no select has run on this object")
        dst, row_bytes = _row_move("PointPopulation.compact", self.n, "select", src, dst)
        word = None
        if fill is not None:
            bits = int(np.float32(fill).view(np.uint32)) if isinstance(fill, (float, np.floating)) else int(fill) & 0xFFFFFFFF
            word = C.byref(C.c_uint32(bits))
        if self.n:
            _raise(lib.hns_point_population_compact(ptr, src.data_ptr(), dst.data_ptr(), row_bytes, word))
        return dst

    @staticmethod
    def _birth_rows(what, xyz, voxel):
        _xyz3(what, xyz, "a (rows, 3)")
        rows = int(xyz.shape[0])
        if voxel is not None and (voxel.dtype != _torch().int32 or tuple(voxel.shape) != (rows,)):
            raise ValueError(f"{what}: voxel must be an int32 tensor of one word per row of xyz")
        return rows, (_ptr(xyz) if rows else 0), (_ptr(voxel) if voxel is not None and rows else 0)

    def birth(self, field, xyz, masks=None, voxel=None, *, threshold: float, rate: float, max_per_voxel: int, seed: int, append: bool = False, fill: bool = True,
              stream: Optional[int] = None):
        """Points from a field: every voxel of `field` ((voxels,) float32 on the object's grid) above `threshold` -- and, with masks ((leaves, 64) uint8 device tensor), active
        -- bears min(value * rate, max_per_voxel) points, the fraction rounded up with that probability by a hash of the voxel's coordinates and `seed`, at hashed positions
        inside the voxel, in voxel order, into the rows of xyz ((rows, 3) float32) from the live count on (append) or from 0; voxel (None or (rows,) int32) receives each
        birth's flat voxel index. Rows at or beyond len(xyz) are dropped; ``counts`` tells (live, wanted). fill: the rows from the live count on become NaN / -1. Equal in
        every byte to ``leafio.birth_points``. Returns self."""
        rows, px, pv = self._birth_rows("PointPopulation.birth", xyz, voxel)
        spec = leafio.birth_spec(threshold, rate, max_per_voxel, seed, fill)
        _raise(lib.hns_point_population_birth(self._bind(stream), _ptr(field), _byte_ptr(masks), C.byref(spec), px, pv, rows, int(bool(append))))
        return self

    def counts(self):
        """(live, wanted): waits for the bound stream. wanted above live: the last birth did not fit its rows"""
        live, wanted = C.c_uint64(0), C.c_uint64(0)
        _raise(lib.hns_point_population_counts(self._live(), C.byref(live), C.byref(wanted)))
        return int(live.value), int(wanted.value)


MOTION_MODES = {"free": _lib.HNS_MOTION_FREE, "stick": _lib.HNS_MOTION_STICK, "bounce": _lib.HNS_MOTION_BOUNCE, "kill": _lib.HNS_MOTION_KILL}
MOTION_HIT = {"bounced": 1, "reverted": 2, "killed": 4, "started_inside": 8, "reflected": 16}  # the bits of PointMotion.hit


class PointMotion(_Handle):
    """Points with a velocity of their own on the device (``hns_point_motion``; include/hns.h states the arithmetic line by line): embers, sparks, soot, debris. The object
    OWNS the per-point state -- ``xyz`` [capacity, 3] (index space), ``vel`` [capacity, 3] (the units of the sim's velocity), ``age``, ``status`` and ``hit`` [capacity] --
    in one block of the pool of device memory; the attributes are torch views of the library's arrays, valid until ``close``: fill xyz, vel and age through them.
    ``step`` drags every point towards a sim's gas, lets it fall, moves it, and answers a step that lands in the sim's "collision_sdf" by `mode`. Bound to no grid: a
    step uses the grid the sim has at that call, so the object survives regrids. A row with a non-finite xyz (``PointPopulation``'s rows beyond the live count) is not
    stepped."""

    _destroy = "hns_point_motion_destroy"

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"PointMotion: capacity {capacity} is negative")
        self.capacity = capacity
        self._create(lib.hns_point_motion_create, capacity)

    def _view(self, which: str, shape, typestr: str):
        info = _lib.hns_point_motion_info()
        _raise(lib.hns_point_motion_get(self._live(), C.byref(info)))
        torch = _torch()
        if self.capacity == 0:
            return torch.empty(shape, dtype=torch.float32 if typestr == "<f4" else torch.uint8, device="cuda")
        return torch.as_tensor(_DeviceWords(getattr(info, which), 0, self, shape, typestr), device="cuda")

    @property
    def xyz(self):
        """positions, [capacity, 3] float32 in index space -- a view of the object's array, valid until ``close``; no wait"""
        return self._view("xyz", (self.capacity, 3), "<f4")

    @property
    def vel(self):
        """the points' own velocities, [capacity, 3] float32 in the units of the sim's velocity -- a view, valid until ``close``; no wait"""
        return self._view("vel", (self.capacity, 3), "<f4")

    @property
    def age(self):
        """[capacity] float32 -- a view, valid until ``close``; no wait"""
        return self._view("age", (self.capacity,), "<f4")

    @property
    def status(self):
        """[capacity] uint8, what the last ``step`` left: 1 alive, finite, inside a leaf and younger than max_age -- a view, valid until ``close``; no wait"""
        return self._view("status", (self.capacity,), "|u1")

    @property
    def hit(self):
        """[capacity] uint8, what the last ``step`` left: MOTION_HIT's bits ORed over its steps -- a view, valid until ``close``; no wait"""
        return self._view("hit", (self.capacity,), "|u1")

    def step(self, sim, n: int, dt: float, voxel_size: float, steps: int = 1, mode: str = "bounce", gravity=(0.0, 0.0, 0.0), drag: float = 0.0, restitution: float = 0.5,
             friction: float = 0.0, max_age: float = float("inf"), threshold: float = 0.0, skin: float = 1 / 16, iterations: int = 3, stream: Optional[int] = None):
        """`steps` steps of rows 0 .. n - 1 in one launch (``hns_point_motion_step``): v = (v + drag*dt*U(x)) / (1 + drag*dt) (implicit Euler towards the gas's velocity
        U), v += dt*gravity, x += (dt / voxel_size)*v, age += dt; then, unless mode is "free", a step that ends where the SDF's sample is below `threshold` puts the point
        back with zero velocity ("stick"), reflects the velocity about the SDF's normal -- `restitution` of the normal speed back, `friction` of the tangential velocity
        lost -- and pushes the point out as ``trace_points_collide`` does, up to `iterations` times ("bounce"), or marks it dead ("kill"). Afterwards ``status`` is 1 where
        the point is alive, finite, inside a leaf and younger than `max_age` -- ``PointPopulation.select(motion.status, 1)`` drops the rest -- and ``hit`` ORs MOTION_HIT.
        The sim is only read. stream: a hipStream_t as an integer, None = torch's current stream; the step is asynchronous on it. Returns self."""
        ptr = self._live()
        if mode not in MOTION_MODES:
            raise ValueError(f"PointMotion.step: mode must be one of {sorted(MOTION_MODES)}, not {mode!r}")
        g = tuple(float(c) for c in gravity)
        if len(g) != 3:
            raise ValueError("PointMotion.step: gravity has three components")
        spec = _lib.hns_point_motion_spec(MOTION_MODES[mode], (C.c_float * 3)(*g), float(drag), float(restitution), float(friction), float(max_age), float(threshold),
                                          float(skin), int(iterations))
        _raise(lib.hns_point_motion_set_stream(ptr, _stream(stream)))
        _raise(lib.hns_point_motion_step(ptr, sim._ptr, int(n), float(dt), float(voxel_size), int(steps), C.byref(spec)))
        return self

    def close(self) -> None:
        """the block goes back to the pool (which waits for the device first); the views must not be used afterwards"""
        super().close()


class Shaping(_Handle):
    """Shaping a device-resident sim in place (``hns_shaping``; include/hns.h states the arithmetic line by line): divergence-free curl-noise turbulence on the velocity,
    optionally weighted by a control field, and implicit decay of float fields towards a target, in one launch over the sim's leaves. The object holds no device memory
    and is bound to no sim: ``apply`` takes the sim."""

    TURBULENCE = dict(amplitude=0.0, frequency=1.0 / 16, offset=(0.0, 0.0, 0.0), octaves=1, lacunarity=2.0, gain=0.5, seed=0, control=None, control_lo=0.0, control_hi=1.0)

    _destroy = "hns_shaping_destroy"

    def __init__(self):
        self._create(lib.hns_shaping_create)

    @classmethod
    def turbulence_spec(cls, turbulence: dict):
        """the ``hns_turbulence_spec`` of a dict with the keys of ``Shaping.TURBULENCE`` (missing ones take its values)"""
        unknown = set(turbulence) - set(cls.TURBULENCE)
        if unknown:
            raise ValueError(f"Shaping: unknown turbulence keys {sorted(unknown)} (known: {sorted(cls.TURBULENCE)})")
        t = {**cls.TURBULENCE, **turbulence}
        off = tuple(float(c) for c in t["offset"])
        if len(off) != 3:
            raise ValueError("Shaping: offset has three components")
        return _lib.hns_turbulence_spec(float(t["amplitude"]), float(t["frequency"]), (C.c_float * 3)(*off), int(t["octaves"]), float(t["lacunarity"]), float(t["gain"]),
                                        int(t["seed"]) & 0xFFFFFFFF, None if t["control"] is None else str(t["control"]).encode(), float(t["control_lo"]),
                                        float(t["control_hi"]))

    def apply(self, sim, dt: float, turbulence: Optional[dict] = None, decay: Optional[dict] = None, stream: Optional[int] = None):
        """One launch on `sim` (``hns_shaping_apply``). turbulence: None, or a dict with the keys of ``Shaping.TURBULENCE`` -- v += amplitude * dt * w * C, C the summed
        curl of `octaves` octaves of gradient noise at `frequency` lattice cells per voxel (each octave `lacunarity` times finer and `gain` times weaker; one octave has
        |C| about 0.8 on average), w = 1 or, with `control` the name of a float field, clamp((field - control_lo) / (control_hi - control_lo), 0, 1) of its value before
        this call's decay; scroll `offset` to animate. decay: None, or {name: (rate, target)} of up to eight float fields -- f = target + (f - target) / (1 + rate * dt).
        stream: a hipStream_t as an integer, None = torch's current stream; the call is asynchronous on it. Returns self."""
        ptr = self._live()
        spec = None if turbulence is None else self.turbulence_spec(turbulence)
        rows = list((decay or {}).items())
        arr = (_lib.hns_decay_spec * max(1, len(rows)))()
        for d, (name, (rate, target)) in zip(arr, rows):
            d.name, d.rate, d.target = str(name).encode(), float(rate), float(target)
        _raise(lib.hns_shaping_set_stream(ptr, _stream(stream)))
        _raise(lib.hns_shaping_apply(ptr, sim._ptr, float(dt), None if spec is None else C.byref(spec), arr if rows else None, len(rows)))
        return self


def shaping_curl_host(turbulence: dict, ijk) -> np.ndarray:
    """C of the voxels `ijk` ([n, 3] int32 global coordinates), [n, 3] float32, evaluated on the host by ``hns_shaping_curl_host`` -- the summed curl before amplitude,
    control and dt, from the header the kernel includes. Needs no device."""
    spec = Shaping.turbulence_spec(turbulence)
    ijk = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
    out = np.empty((len(ijk), 3), np.float32)
    one = _lib.hns_shaping_curl()
    fn, ref = lib.hns_shaping_curl_host, C.byref(one)
    for r, (i, j, k) in enumerate(ijk.tolist()):
        _raise(fn(C.byref(spec), i, j, k, ref))
        out[r] = one.c[0], one.c[1], one.c[2]
    return out


class Diffusion(_Handle):
    """Implicit diffusion of float fields and viscosity of the velocity on a device-resident sim (``hns_diffusion``; include/hns.h states the arithmetic line by line):
    per field (I - a L) x = b over the sim's unknowns, a = coefficient * dt / voxel_size**2, by a fixed number of Jacobi or Chebyshev iterations, one launch each. The
    object holds its stream and the pooled scratch of its calls and is bound to no sim: ``apply`` takes the sim."""

    METHODS = {"jacobi": _lib.HNS_DIFFUSION_JACOBI, "chebyshev": _lib.HNS_DIFFUSION_CHEBYSHEV}

    _destroy = "hns_diffusion_destroy"

    def __init__(self):
        self._create(lib.hns_diffusion_create)

    @classmethod
    def spec(cls, viscosity: float = 0.0, iterations: int = 8, method: str = "jacobi", collide: bool = False, threshold: float = 0.0):
        """the ``hns_diffusion_spec`` of these arguments"""
        if method not in cls.METHODS:
            raise ValueError(f"Diffusion: unknown method {method!r} (known: {sorted(cls.METHODS)})")
        return _lib.hns_diffusion_spec(int(iterations), cls.METHODS[method], float(viscosity), 1 if collide else 0, float(threshold))

    def apply(self, sim, dt: float, voxel_size: float, fields: Optional[dict] = None, viscosity: float = 0.0, iterations: int = 8, method: str = "jacobi",
              collide: bool = False, threshold: float = 0.0, stream: Optional[int] = None):
        """``hns_diffusion_apply`` on `sim`. fields: None, or {name: coefficient} of up to eight float fields; viscosity: the velocity's coefficient (0: the velocity
        is neither read nor written); iterations 1 .. 256 of method "jacobi" or "chebyshev"; collide: voxels whose ``collision_sdf`` lies below `threshold` are solid --
        zero-flux for a float field, a no-slip wall at rest for the velocity. Only the sim's unknowns (active, not solid) are written. stream: a hipStream_t as an integer,
        None = torch's current stream; the call is asynchronous on it. Returns self."""
        ptr = self._live()
        spec = self.spec(viscosity, iterations, method, collide, threshold)
        rows = list((fields or {}).items())
        unknown = [str(k) for k, _ in rows if str(k) not in sim.names]
        if unknown:
            raise ValueError(f"Diffusion: unknown fields {sorted(unknown)} (the sim's float fields: {sorted(sim.names)})")
        arr = (_lib.hns_diffusion_term * max(1, len(rows)))()
        for t, (name, coefficient) in zip(arr, rows):
            t.name, t.coefficient = str(name).encode(), float(coefficient)
        _raise(lib.hns_diffusion_set_stream(ptr, _stream(stream)))
        _raise(lib.hns_diffusion_apply(ptr, sim._ptr, float(dt), float(voxel_size), C.byref(spec), arr if rows else None, len(rows)))
        return self


def diffusion_schedule_host(coefficient: float, dt: float, voxel_size: float, iterations: int) -> dict:
    """The host constants of one coefficient (``hns_diffusion_schedule_host``; needs no device): {"a": float32, "r": float32[7], "rho": float32,
    "omega": float32[256]}, omega[k - 1] = w_k for k <= iterations and 0 behind them."""
    out = _lib.hns_diffusion_schedule()
    _raise(lib.hns_diffusion_schedule_host(float(coefficient), float(dt), float(voxel_size), int(iterations), C.byref(out)))
    return {"a": np.float32(out.a), "r": np.array(out.r[:], np.float32), "rho": np.float32(out.rho), "omega": np.array(out.omega[:], np.float32)}


def stats_buffer(n_records: int = 1):
    """Device memory for `n_records` hns_stats records (a uint8 tensor; ``read_stats`` brings it to the host)."""
    return _torch().zeros(n_records * leafio.STATS_DTYPE.itemsize, dtype=_torch().uint8, device="cuda")


def read_stats(buf) -> np.ndarray:
    """The records of a ``stats_buffer`` on the host (waits for the current stream): an array of leafio.STATS_DTYPE"""
    return buf.cpu().numpy().view(leafio.STATS_DTYPE).copy()


def field_stats(grid: IndexGridHandle, values, masks=None, out=None):
    """Statistics of a field in device memory over all leaves of `grid` (``hns_dev_field_stats``): values (N,) or (N, 3) float32, masks a uint8 tensor of
    leaf_count x 64 bytes or None = every voxel. One record per component into `out` (``stats_buffer``), asynchronous on the current stream."""
    ncomp = 3 if (values.dim() == 2 and values.shape[1] == 3) else 1
    out = stats_buffer(ncomp) if out is None else out
    _raise(lib.hns_dev_field_stats(grid.ptr, _ptr(values), ncomp, _byte_ptr(masks), _byte_ptr(out), current_stream()))
    return out


def residual(grid: IndexGridHandle, div, p, dx: float, c_out=None, out=None):
    """The Gauss-Seidel correction c of pressure `p` against `div` over the grid's launch range (``hns_dev_residual``): its record into `out`
    (``stats_buffer``), the field itself into c_out when given. Asynchronous on the current stream. ``residual_in_divergence_units`` rescales."""
    out = stats_buffer(1) if out is None else out
    _raise(lib.hns_dev_residual(grid.ptr, _ptr(div), _ptr(p), dx, _ptr(c_out), _byte_ptr(out), current_stream()))
    return out


def residual_in_divergence_units(c, dx: float):
    """-6 c / dx^2: a correction (a value, or the min / max / max_abs of a record) as a residual of the discrete Poisson equation, in the divergence's units"""
    return -6.0 * c / (dx * dx)


def _record(r) -> np.ndarray:
    return np.frombuffer(bytes(r), dtype=leafio.STATS_DTYPE).copy()


def _leaf_source(entry, leaves, need, keep, ncomp: Optional[int] = None) -> None:
    """Fills the hns_leaf_source `entry` (all but its name) from (origins, masks or None, values) of the collision SDF or a regrid source: the
    arrays contiguous, their sizes checked against the origins, kept alive in `keep`. ncomp None: 3 for values of shape (n * 512, 3), else 1.
    need: how the values and the masks refusals begin."""
    so, sm, sv = leaves
    o = np.ascontiguousarray(so, dtype=np.int32).reshape(-1, 3)
    v = np.ascontiguousarray(sv, dtype=np.float32)
    nc = ncomp or (3 if (v.ndim == 2 and v.shape[1] == 3) else 1)
    if v.size != len(o) * 512 * nc:
        per_leaf = "512" if ncomp else f"512 x {nc}"
        raise ValueError(f"{need[0]} {len(o)} x {per_leaf} floats, got {v.size}")
    m = None if sm is None else np.ascontiguousarray(sm, dtype=np.uint8).reshape(-1)
    if m is not None and m.size != len(o) * 64:
        raise ValueError(f"{need[1]} {len(o)} x 64 bytes, got {m.size}")
    keep += [o, m, v]
    entry.ncomp, entry.origins, entry.n_leaves, entry.values = nc, o.ctypes.data, len(o), v.ctypes.data
    entry.masks = None if m is None else m.ctypes.data


class Sim(_Handle):
    """Device-resident simulation state (``hns_sim``): upload once, run many substeps."""

    _destroy = "hns_sim_destroy"

    def __init__(self, grid: IndexGridHandle, float_names: Sequence[str]):
        self.grid = grid
        self.names = list(float_names)
        self._shaping = None  # the Shaping that ``shape`` makes on first use
        self._diffusion = None  # the Diffusion that ``diffuse`` makes on first use
        self._create(lib.hns_sim_create, grid.ptr, _names(self.names), len(self.names))

    def _fields(self, arrays: dict):
        arr = (hns_field * max(1, len(arrays)))()
        keep = []
        for i, (name, a) in enumerate(arrays.items()):
            if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"]:
                raise TypeError(f"{name}: need C-contiguous float32")
            b = name.encode()
            keep.append(b)
            arr[i].name = b
            arr[i].ncomp = 3 if (a.ndim == 2 and a.shape[1] == 3) else 1
            arr[i].host = a.ctypes.data_as(C.POINTER(C.c_float))
        return arr, len(arrays), keep

    def upload(self, arrays: dict, stream: Optional[int] = None) -> None:
        arr, n, keep = self._fields(arrays)
        _raise(lib.hns_sim_upload(self._ptr, arr, n, stream or 0))

    def download(self, arrays: dict, stream: Optional[int] = None) -> None:
        arr, n, keep = self._fields(arrays)
        _raise(lib.hns_sim_download(self._ptr, arr, n, stream or 0))

    def substep(self, iterations: int, dt: float, voxel_size: float, params: CombustionParams, has_collision: bool = False, stream: int = 0) -> None:
        p = params._c()
        _raise(lib.hns_sim_substep(self._ptr, iterations, dt, voxel_size, C.byref(p), int(has_collision), stream))

    def core_substep(self, iterations: int, dt: float, voxel_size: float, stream: int = 0) -> None:
        _raise(lib.hns_sim_core_substep(self._ptr, iterations, dt, voxel_size, stream))

    def advect(self, names: Optional[Sequence[str]] = None, velocity: bool = False, *, dt: float, voxel_size: float, stream: int = 0) -> None:
        """AdvectIndexGrid over the float fields `names` (None: all of them) with the current velocity, then, with `velocity`, AdvectIndexGridVelocity
        (``hns_sim_advect``). Asynchronous on `stream`; an unknown or repeated name is refused with nothing changed."""
        if names is None:
            _raise(lib.hns_sim_advect(self._ptr, None, -1, int(velocity), dt, voxel_size, stream))
            return
        _raise(lib.hns_sim_advect(self._ptr, _names(names), len(names), int(velocity), dt, voxel_size, stream))

    def sample(self, names: Optional[Sequence[str]] = None, xyz=None, velocity: bool = False, stream: Optional[int] = None) -> dict:
        """The sim's float fields `names` (None: all of them) and, with `velocity`, its velocity under the key "vel", at the positions xyz ((n, 3) float32 device
        tensor, index space): {name: tensor} (``hns_sim_sample_points``). Asynchronous on `stream` (None: the current stream); the sim is only read."""
        if xyz is None:
            raise ValueError("Sim.sample: xyz is required")
        names = list(self.names) if names is None else list(names)
        n, t = xyz.shape[0], _torch()
        out = {k: t.empty(n, dtype=t.float32, device=xyz.device) for k in names}
        if len(out) != len(names):
            raise ValueError("Sim.sample: a name is listed twice")
        if velocity:
            out["vel"] = t.empty((n, 3), dtype=t.float32, device=xyz.device)
        _raise(lib.hns_sim_sample_points(self._ptr, _names(names), len(names), int(velocity), _ptr(xyz), n, _ptrs(out.values()), _stream(stream)))
        return out

    def trace(self, xyz, *, dt: float, voxel_size: float, order: int = 2, steps: int = 1, status: bool = False, stream: Optional[int] = None, collide: Optional[str] = None,
              threshold: float = 0.0, skin: float = 1 / 16, iterations: int = 2, hit: bool = False):
        """`steps` steps of the points xyz (moved in place) through the sim's current velocity (``hns_sim_trace_points``); with `status` returns the uint8 tensor
        that is 1 where a point ended finite and inside a leaf. Asynchronous on `stream` (None: the current stream); the sim is only read.
        collide: None, or "stop", "push" or "kill": the sim's field collision_sdf is tested after every step (``hns_sim_trace_points_collide``, ``trace_points_collide``
        for threshold, skin and iterations); with `hit` the return value is (status or None, the uint8 tensor of hit bits)."""
        spec = None if collide is None else _collision("Sim.trace", collide, threshold, skin, iterations)
        t = _torch()
        st = t.empty(xyz.shape[0], dtype=t.uint8, device=xyz.device) if status else None
        stream = _stream(stream)
        if spec is None:
            if hit:
                raise ValueError("Sim.trace: hit needs collide")
            _raise(lib.hns_sim_trace_points(self._ptr, _ptr(xyz), xyz.shape[0], dt, voxel_size, int(order), int(steps), _byte_ptr(st), stream))
            return st
        ht = t.empty(xyz.shape[0], dtype=t.uint8, device=xyz.device) if hit else None
        _raise(lib.hns_sim_trace_points_collide(self._ptr, _ptr(xyz), xyz.shape[0], dt, voxel_size, int(order), int(steps), C.byref(spec), _byte_ptr(st), _byte_ptr(ht),
                                                stream))
        return (st, ht) if hit else st

    def splat(self, values: dict, xyz, velocity=None, log2_quantum: int = -32, activate: bool = True, status: bool = False, rejected=None, stream: Optional[int] = None, *,
              kernel: str = "trilinear", mode: str = "add", radius=None, max_radius: Optional[float] = None, min_weight: float = 0.0, order: Optional[PointOrder] = None,
              rows: str = "original"):
        """Point values added into the sim's own fields (``hns_sim_splat_points``, the arithmetic of ``splat_points``): values = {float field name: (n,) float32 device
        tensor}, velocity = None or an (n, 3) tensor added into the velocity, xyz the (n, 3) index-space positions. activate: on a sim that holds active masks, set the bit
        of every voxel a tap of positive weight landed on. Points outside the domain add no leaves: with `status` the uint8 tensor of landed taps per point (0 .. 8) is
        returned. rejected: None or an int64 tensor of one element, as for ``splat_points``. kernel, mode, radius, max_radius, min_weight: as for ``splat_points`` (the
        spec is stored with the sim for the call). Asynchronous on `stream` (None: the current stream).
        order: a ``PointOrder`` on the sim's grid whose last sort saw these points: the call goes through it (``hns_point_order_splat_sim``: leaves summed on chip, the
        same bytes, masks and status) on the stream of that sort -- `stream` must then be None --; rows as for ``PointOrder.splat``."""
        names = list(values)
        if order is None:
            if rows != "original":
                raise ValueError("Sim.splat: rows is about an order; without one the arrays are what they are")
        else:
            if stream is not None:
                raise ValueError("Sim.splat: an order runs on the stream of its last sort; pass no stream with it")
            if order.grid is not self.grid:
                raise ValueError("Sim.splat: the order was made on another grid than the sim's current one")
            r = order._splat_rows("Sim.splat", rows, xyz, [(k, values[k]) for k in names] + [("velocity", velocity)])
        spec = splat_spec(kernel, mode, radius, max_radius, min_weight, pointer=lambda t: _radius_ptr(t, xyz.shape[0]))
        st = _torch().empty(xyz.shape[0], dtype=_torch().uint8, device=xyz.device) if status else None
        arr, src = _names(names), _ptrs(values[k] for k in names)
        if order is not None:
            with stored_splat_spec(lib.hns_sim_set_splat_spec, lib.hns_sim_get_splat_spec, self._ptr, spec):
                _raise(lib.hns_point_order_splat_sim(order._live(), self._ptr, arr, len(names), _ptr(velocity), _ptr(xyz) if order.n else 0, src, r, int(log2_quantum),
                                                     int(bool(activate)), _byte_ptr(st), _u64_ptr(rejected)))
            return st
        with stored_splat_spec(lib.hns_sim_set_splat_spec, lib.hns_sim_get_splat_spec, self._ptr, spec):
            _raise(lib.hns_sim_splat_points(self._ptr, arr, len(names), _ptr(velocity), _ptr(xyz), src, xyz.shape[0], int(log2_quantum), int(bool(activate)),
                                            _byte_ptr(st), _u64_ptr(rejected), _stream(stream)))
        return st

    def pressure_solve(self, iterations: int, voxel_size: float, stream: int = 0) -> None:
        _raise(lib.hns_sim_pressure_solve(self._ptr, iterations, voxel_size, stream))

    def timing(self, max_solves: int) -> None:
        _raise(lib.hns_sim_timing(self._ptr, max_solves))

    def pressure_time(self):
        """(total ms of the event-bracketed pressure loops, number of fused-iteration launches inside them)"""
        ms, n = C.c_float(0.0), C.c_longlong(0)
        _raise(lib.hns_sim_pressure_time(self._ptr, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def stage_timing(self, max_substeps: int) -> None:
        _raise(lib.hns_sim_stage_timing(self._ptr, max_substeps))

    def stage_times(self):
        """({stage: total ms} over the core substeps timed since timing(), number of substeps)"""
        ms, n = (C.c_float * 5)(), C.c_longlong(0)
        _raise(lib.hns_sim_stage_times(self._ptr, ms, C.byref(n)))
        return dict(zip(("advect_vector", "divergence", "pressure", "gradient", "advect_scalars"), [float(x) for x in ms])), int(n.value)

    def lookahead_counts(self):
        """(substeps that launched the look-ahead form of advect_scalars, substeps that skipped their advect_vector launch for it)"""
        p, c = C.c_longlong(0), C.c_longlong(0)
        _raise(lib.hns_sim_lookahead_counts(self._ptr, C.byref(p), C.byref(c)))
        return int(p.value), int(c.value)

    def substep_plan(self, params: Optional[CombustionParams] = None, has_collision: bool = False) -> dict:
        """{stage: kernel form} of the next ``substep`` (params None: ``core_substep``) with these arguments (``hns_sim_substep_plan``); launches nothing.
        Stages: collision advect_vector vorticity divergence pressure gradient advect_scalars; "-" = no launch, "memo" = already looked ahead."""
        buf = C.create_string_buffer(1024)
        p = None if params is None else params._c()
        _raise(lib.hns_sim_substep_plan(self._ptr, None if p is None else C.byref(p), int(has_collision), buf, 1024))
        return dict(w.split("=", 1) for w in buf.value.decode().split())

    def velocity_ptr(self) -> int:
        """Raw device pointer of the velocity (``hns_sim_velocity_ptr``): writable, so the sim stops looking ahead."""
        return int(lib.hns_sim_velocity_ptr(self._ptr) or 0)

    def set_active_masks(self, masks: Optional[np.ndarray], stream: int = 0) -> None:
        """Active voxel masks of the grid's leaves (leaf_count x 64 uint8, byte x*8+y, bit z); None = every voxel active (a new sim's state)."""
        if masks is None:
            _raise(lib.hns_sim_set_active_masks(self._ptr, None, stream))
            return
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.size != self.grid.leaf_count() * 64:
            raise ValueError(f"masks: need {self.grid.leaf_count()} x 64 bytes, got {m.size}")
        _raise(lib.hns_sim_set_active_masks(self._ptr, m.ctypes.data, stream))

    def active_masks(self, stream: int = 0) -> np.ndarray:
        out = np.empty((self.grid.leaf_count(), 64), dtype=np.uint8)
        _raise(lib.hns_sim_active_masks(self._ptr, out.ctypes.data, stream))
        return out

    last_seeds_skipped = 0  # points of the last regrid(points=...) that did not seed

    def regrid(self, padding: int, sdf=None, sources=None, points=None, stream: int = 0) -> IndexGridHandle:
        """The domain change between two cooks (``hns_sim_regrid``): dilate the active masks by `padding` voxels, unite with the collision SDF's
        leaves and carry every field into the new leaf set, on the device. sdf = (origins, masks or None, values: 512 floats per leaf) or None.
        sources = {name: (origins, masks or None, values)}: this frame's sources, added into the fields first (``hns_sim_regrid_sourced``); values
        of shape (n * 512, 3) make the source the velocity's, anything else holds 512 floats per leaf of a float field.
        points = an (n, 3) float32 device tensor of index-space positions whose seeds (``point_leaves``) join the velocity's topology before the dilation, adding no value
        to any field (``hns_sim_regrid_seeded``): afterwards every tap of every seeding point is inside the domain. ``last_seeds_skipped`` holds the points that did not seed.
        Returns the new grid and makes it ``self.grid``; the old handle is untouched and still the caller's."""
        err, keep = C.c_int(0), []
        sdf_e = _lib.hns_leaf_source()  # (NULL arrays, no leaves: no SDF)
        if sdf is not None:
            _leaf_source(sdf_e, sdf, ("sdf values: need", "sdf masks: need"), keep, 1)
        sdf_args = (sdf_e.origins, sdf_e.n_leaves, sdf_e.masks, sdf_e.values)
        if sources is None and points is None:
            ptr = lib.hns_sim_regrid(self._ptr, int(padding), *sdf_args, stream, C.byref(err))
        else:
            sources = sources or {}
            arr = (_lib.hns_leaf_source * max(1, len(sources)))()
            for i, (name, leaves) in enumerate(sources.items()):
                keep.append(name.encode())
                arr[i].name = keep[-1]
                _leaf_source(arr[i], leaves, (f"source {name}: need", f"source {name}: masks need"), keep)
            if points is None:
                ptr = lib.hns_sim_regrid_sourced(self._ptr, int(padding), arr, len(sources), *sdf_args, stream, C.byref(err))
            else:
                if points.dim() != 2 or points.shape[1] != 3:
                    raise ValueError("regrid: points must be an (n, 3) tensor")
                n, skipped = int(points.shape[0]), C.c_uint64(0)
                ptr = lib.hns_sim_regrid_seeded(self._ptr, int(padding), arr, len(sources), _ptr(points) if n else 0, n, C.byref(skipped), *sdf_args, stream, C.byref(err))
                self.last_seeds_skipped = int(skipped.value)
        if not ptr:
            _raise(err.value if err.value < 0 else _lib.HNS_ERR_RUNTIME)
        self.grid = IndexGridHandle(ptr)
        return self.grid

    def emit(self, values: dict, xyz, velocity=None, *, padding: int = 1, sdf=None, sources=None, log2_quantum: int = -32, rejected=None, stream: int = 0,
             kernel: Optional[str] = None, mode: str = "add", radius=None, max_radius: Optional[float] = None, min_weight: float = 0.0):
        """A point emitter's frame step without a host round trip: ``regrid(padding, sdf, sources, points=xyz)``, which makes room for every tap of every seeding point,
        then ``splat(values, xyz, velocity, activate=True, status=True)`` on the new domain -> (the new grid, the uint8 status tensor: 8 for every seeding point).
        With a `radius` the splat is radial (kernel, mode, radius, max_radius, min_weight: as for ``splat``) and the status of every seeding point is 2; the seeds are still
        the eight taps of each point's cell, and a footprint voxel lies within ceil(radius) voxels of that cell along every axis, so `padding` must be at least
        ceil(the largest radius): the regrid's dilation by `padding` then covers the footprint. Anything less raises ValueError before anything runs."""
        if kernel is None:
            kernel = "trilinear" if radius is None else "radial"
        if kernel == "radial":
            bound = radius if isinstance(radius, (int, float, np.floating, np.integer)) else max_radius
            if bound is None or not int(padding) >= int(np.ceil(float(bound))):
                raise ValueError(f"emit: a radial splat needs padding >= ceil(the largest radius): padding {padding}, radius bound {bound}")
        grid = self.regrid(padding, sdf, sources, points=xyz, stream=stream)
        status = self.splat(values, xyz, velocity, log2_quantum=log2_quantum, activate=True, status=True, rejected=rejected, stream=stream, kernel=kernel, mode=mode,
                            radius=radius, max_radius=max_radius, min_weight=min_weight)
        return grid, status

    def deactivate(self, tolerances: dict, velocity: Optional[float] = None, counts: bool = False, stream: int = 0):
        """The end of a frame (``hns_sim_deactivate``): clear the active bit of every voxel whose listed components are all within tolerance
        (|x| <= tol; NaN never is). tolerances = {float field name: tolerance}; velocity = the velocity's tolerance, None = not tested. Field values
        are untouched; the next regrid drops the leaves no active voxel reaches, with all their values. Asynchronous on `stream`, unless counts:
        then synchronous, returning (active voxels, leaves holding one)."""
        arr, n = leafio.activity_fields(tolerances, velocity)
        out = (C.c_uint64 * 2)()
        _raise(lib.hns_sim_deactivate(self._ptr, arr, n, out if counts else None, stream))
        return (int(out[0]), int(out[1])) if counts else None

    def stats(self, names: Sequence[str], velocity: bool = False, masks: bool = True, stream: int = 0) -> np.ndarray:
        """Statistics of float fields `names` and, with velocity, of the velocity's three components behind them (``hns_sim_stats``): one record
        (leafio.STATS_DTYPE) per component, over the active voxels (masks) or all of them. Synchronous; equal in every byte to ``leafio.leaf_stats`` of the
        downloaded fields. dt * max(max_abs of the velocity's records) / dx is the longest back-trace in voxels."""
        entries = [(n.encode(), 1) for n in names] + ([(None, 3)] if velocity else [])
        arr = (_lib.hns_stats_field * max(1, len(entries)))()
        for i, (name, nc) in enumerate(entries):
            arr[i].name, arr[i].ncomp = name, nc
        out = np.zeros(sum(nc for _, nc in entries), dtype=leafio.STATS_DTYPE)
        _raise(lib.hns_sim_stats(self._ptr, arr, len(entries), int(masks), out.ctypes.data, stream))
        return out

    def residual(self, voxel_size: float, stream: int = 0) -> np.ndarray:
        """The record of the Gauss-Seidel correction of the last pressure solve (``hns_sim_residual``); ``residual_in_divergence_units`` rescales it."""
        r = _lib.hns_stats()
        _raise(lib.hns_sim_residual(self._ptr, voxel_size, C.byref(r), stream))
        return _record(r)

    def solve_control(self, rel_tol: Optional[float] = 0.0, abs_tol: float = 0.0, check_every: int = 10) -> None:
        """A stop rule for the pressure solve of pressure_solve / substep / core_substep (``hns_sim_set_solve_control``): their `iterations` becomes the
        maximum and the loop ends at the first check, taken every check_every iterations, where the residual's max_abs <= max(abs_tol, rel_tol * the one
        at p = 0). Both tolerances 0: monitor only. rel_tol None switches the control off."""
        if rel_tol is None:
            _raise(lib.hns_sim_set_solve_control(self._ptr, None))
            return
        c = _lib.hns_solve_control(float(rel_tol), float(abs_tol), int(check_every))
        _raise(lib.hns_sim_set_solve_control(self._ptr, C.byref(c)))

    def solve_report(self) -> dict:
        """What the last controlled solve did (``hns_sim_solve_report``): iterations, checks, converged, initial, final and the history of the checks"""
        r, n = _lib.hns_solve_report(), C.c_int(0)
        _raise(lib.hns_sim_solve_report(self._ptr, C.byref(r), None, 0, C.byref(n)))
        hist = np.zeros(n.value, dtype=leafio.STATS_DTYPE)
        _raise(lib.hns_sim_solve_report(self._ptr, C.byref(r), hist.ctypes.data, n.value, C.byref(n)))
        return {"iterations": r.iterations, "checks": r.checks, "converged": bool(r.converged), "initial": _record(r.initial)[0], "final": _record(r.final)[0],
                "history": hist}

    def solve_method(self, method: Optional[int] = 1, pre: int = 2, post: int = 2, coarse_iterations: int = 8, max_levels: int = 0, omega: float = 1.0) -> None:
        """The solve method of pressure_solve / substep / core_substep (``hns_sim_set_solve_method``). method 1: geometric multigrid V(pre, post) cycles on the
        leaf-sparse grid with exact coarse-level masks -- `iterations` of those calls then counts CYCLES, also under a ``solve_control`` --, `coarse_iterations` sweeps on the
        coarsest level, at most `max_levels` levels (0: as deep as the leaf set goes), every sweep relaxed by `omega`. method 0 or None: back to SOR, the default."""
        if method is None:
            _raise(lib.hns_sim_set_solve_method(self._ptr, None))
            return
        m = _lib.hns_solve_method(int(method), int(pre), int(post), int(coarse_iterations), int(max_levels), float(omega))
        _raise(lib.hns_sim_set_solve_method(self._ptr, C.byref(m)))

    def solve_levels(self) -> List[int]:
        """Leaves per level of the V-cycle's hierarchy, level 0 first (``hns_sim_solve_levels``)"""
        n = C.c_int(0)
        _raise(lib.hns_sim_solve_levels(self._ptr, C.byref(n), None, 0))
        out = (C.c_uint64 * max(1, n.value))()
        _raise(lib.hns_sim_solve_levels(self._ptr, C.byref(n), out, n.value))
        return [int(x) for x in out[: n.value]]

    def point_order(self, capacity: int) -> PointOrder:
        """A ``PointOrder`` for up to `capacity` points on the sim's CURRENT grid. After a ``regrid`` the sim is on another grid and the object refuses every call
        (RuntimeError): make a new one."""
        return PointOrder(self.grid, capacity, _sim=self)

    def point_population(self, capacity: int) -> PointPopulation:
        """A ``PointPopulation`` for up to `capacity` points on the sim's CURRENT grid. After a ``regrid`` the sim is on another grid and the object refuses every call
        (RuntimeError): make a new one."""
        return PointPopulation(self.grid, capacity, _sim=self)

    def point_motion(self, capacity: int) -> PointMotion:
        """A ``PointMotion`` of `capacity` rows. It is bound to no grid: ``motion.step(sim, ...)`` reads the grid the sim has at that call, after a ``regrid`` too."""
        return PointMotion(capacity)

    def shape(self, dt: float, turbulence: Optional[dict] = None, decay: Optional[dict] = None, stream: Optional[int] = None):
        """``Shaping.apply`` on this sim through a ``Shaping`` the sim owns (made on first use, closed with the sim): curl-noise turbulence on the velocity and decay of
        float fields, in place, in one launch. Returns self."""
        if self._shaping is None:
            self._shaping = Shaping()
        self._shaping.apply(self, dt, turbulence, decay, stream)
        return self

    def diffuse(self, dt: float, voxel_size: float, fields: Optional[dict] = None, viscosity: float = 0.0, iterations: int = 8, method: str = "jacobi",
                collide: bool = False, threshold: float = 0.0, stream: Optional[int] = None):
        """``Diffusion.apply`` on this sim through a ``Diffusion`` the sim owns (made on first use, closed with the sim; it keeps its pooled scratch between calls):
        implicit diffusion of float fields and viscosity of the velocity over the sim's unknowns. Returns self."""
        if self._diffusion is None:
            self._diffusion = Diffusion()
        self._diffusion.apply(self, dt, voxel_size, fields, viscosity, iterations, method, collide, threshold, stream)
        return self

    def birth(self, population: PointPopulation, name: str, xyz, voxel=None, *, threshold: float, rate: float, max_per_voxel: int, seed: int, append: bool = False,
              fill: bool = True, use_masks: bool = True, stream: Optional[int] = None):
        """``PointPopulation.birth`` from the sim's own float field `name` and, with use_masks, its active masks (``hns_point_population_birth_sim``): embers where
        "flame" is high, markers where "fuel" is. The population must be on the sim's current grid. Asynchronous on `stream` (None: the current stream)."""
        if population.grid is not self.grid:
            raise ValueError("Sim.birth: the population was made on another grid than the sim's current one")
        rows, px, pv = population._birth_rows("Sim.birth", xyz, voxel)
        spec = leafio.birth_spec(threshold, rate, max_per_voxel, seed, fill)
        _raise(lib.hns_point_population_birth_sim(population._bind(stream), self._ptr, name.encode(), int(bool(use_masks)), C.byref(spec), px, pv, rows, int(bool(append))))
        return population

    def regrid_times(self):
        """hipEvent split of the last regrid in ms: {candidates, host (origins, sort, grid tables), masks, fields}"""
        ms = (C.c_float * 4)()
        _raise(lib.hns_sim_regrid_times(self._ptr, ms))
        return dict(zip(("candidates", "host", "masks", "fields"), [float(x) for x in ms]))

    def close(self) -> None:
        if self._shaping is not None:
            self._shaping.close()
            self._shaping = None
        if self._diffusion is not None:
            self._diffusion.close()
            self._diffusion = None
        super().close()
