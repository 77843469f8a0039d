"""TEST HELPER of tests/test_population.py (CPU) and tests/test_population_gpu.py: birth and death of points restated in numpy from the text of include/hns.h ("BIRTH AND
DEATH OF POINTS"; never from the C++), one float32 operation per line, and the grids, fields and capacities the calls are run on. The conditions the inputs must meet are
counted by the restatement, never by the code under test.

Select: point i is kept iff flags[i] >= at_least; slot[i] = the number of kept points below i, 0xFFFFFFFF for a dropped one; compact is the stable boolean selection
dst[slot[i]] = src[i], rows live .. n - 1 filled or kept, rows from n on untouched.
Birth: see `counts` and `positions` below, line by line the header's Eligible / Hash / Count / Position / Order."""
from __future__ import annotations

import functools

import numpy as np

import order_cases as oc
from hnanosolver_amd import _lib, api

F = np.float32
U32 = np.uint32
DROPPED = 0xFFFFFFFF
NAN_WORD, NO_VOXEL = 0x7FC00000, 0xFFFFFFFF
XYZ_SENTINEL, VOXEL_SENTINEL = 0xDEADBEEF, 0xDEADBEEF  # what the outputs hold before a call (a NaN pattern no birth and no fill produces)

GRIDS = ("one_leaf", "ragged32_off_origin", "sparse_far", "dense64", "five_leaves", "range_edge")


@functools.lru_cache(maxsize=None)
def origins(name):
    if name == "five_leaves":  # one full tile of four leaves and a part of the next
        o = np.ascontiguousarray(oc.origins("dense64")[:5])
    elif name == "range_edge":  # the last and the first coordinates that may bear points: 8388606 and -8388608 (x = 8388607 is a voxel of the first leaf and may not)
        o = np.array([[8388600, 0, -8388608], [-8388608, 8388600, 16], [0, 0, 0]], dtype=np.int32)
    else:
        o = oc.origins(name)
    o = np.ascontiguousarray(o, dtype=np.int32)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def host_grid(name):
    return api.create_grid_from_leaves(origins(name), oc.VS, _lib.HNS_GRID_HOST_ONLY)


def coordinates(o):
    """global (i, j, k) of every voxel, e = leaf * 512 + (x<<6 | y<<3 | z) -> (V, 3) int64"""
    v = np.arange(512)
    local = np.stack([v >> 6, (v >> 3) & 7, v & 7], -1)
    return (np.asarray(o, dtype=np.int64)[:, None, :] + local[None, :, :]).reshape(-1, 3)


def mask_bits(masks, n_leaves):
    """(L, 64) bytes, byte x*8+y, bit z -> (V,) bool in voxel order; None: every voxel"""
    if masks is None:
        return np.ones(n_leaves * 512, dtype=bool)
    return np.unpackbits(np.asarray(masks, dtype=np.uint8).reshape(n_leaves, 64, 1), axis=2, bitorder="little").reshape(-1).astype(bool)


# ---- the header's rule -------------------------------------------------------------------------------------------------------------------------------------------------


def H(x):
    x = np.asarray(x, dtype=U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def as_u32(c):
    return (np.asarray(c, dtype=np.int64) & 0xFFFFFFFF).astype(U32)


def voxel_hash(seed, ijk):
    h = H(np.full(len(ijk), (int(seed) ^ 0x9E3779B9) & 0xFFFFFFFF, dtype=U32))
    h = H(h ^ as_u32(ijk[:, 0]))
    h = H(h ^ as_u32(ijk[:, 1]))
    return H(h ^ as_u32(ijk[:, 2]))


def U(h, d):
    r = H(h + np.asarray(d, dtype=U32))
    return (r >> U32(8)).astype(F) * F(2.0 ** -24)


def counts(o, field, masks, threshold, rate, K, seed):
    """-> (c (V,) int64, h (V,) uint32, eligible, f (V,) float32: the fraction of m, for the conditions)"""
    ijk = coordinates(o)
    v = np.asarray(field, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        eligible = mask_bits(masks, len(o)) & (v > F(threshold)) & ((ijk >= -8388608) & (ijk <= 8388606)).all(1)
        scaled = np.where(eligible, v, F(0)) * F(rate)
    m = np.maximum(F(0), np.minimum(scaled, F(K)))
    b = m.astype(U32)
    f = m - b.astype(F)
    h = voxel_hash(seed, ijk)
    c = b.astype(np.int64) + (U(h, 0) < f)
    c[~eligible] = 0
    return c, h, eligible, f


def positions(ijk, h, q):
    """the position of birth q of the voxels ijk -> ((n, 3) float32, (n, 3) bool: the coordinates that were clamped)"""
    out, clamped = np.zeros((len(ijk), 3), dtype=F), np.zeros((len(ijk), 3), dtype=bool)
    for a in range(3):
        i = ijk[:, a]
        p = i.astype(F) + U(h, 1 + 3 * q + a)
        top = (i + 1).astype(F)
        clamped[:, a] = ~(p < top)
        out[:, a] = np.where(clamped[:, a], np.nextafter(top, F(-np.inf)), p)
    return out, clamped


def births(o, field, masks, threshold, rate, K, seed):
    """every birth in order -> (xyz (n, 3) float32, voxel (n,) uint32, clamped (n, 3) bool, c)"""
    c, h, _, _ = counts(o, field, masks, threshold, rate, K, seed)
    e = np.repeat(np.arange(len(c)), c)
    q = np.arange(len(e)) - np.repeat(np.cumsum(c) - c, c)
    xyz, clamped = positions(coordinates(o)[e], h[e], q.astype(np.int64))
    return xyz, e.astype(U32), clamped, c


def restate_birth(o, field, masks, *, threshold, rate, max_per_voxel, seed, fill=True, start=0, capacity_rows, xyz=None, voxel=None):
    """the call on outputs that hold `xyz` / `voxel` before it (None: the sentinels) -> (xyz, voxel, live, wanted)"""
    out_x = np.full((capacity_rows, 3), XYZ_SENTINEL, dtype=U32).view(F) if xyz is None else np.array(xyz, dtype=F)
    out_v = np.full(capacity_rows, VOXEL_SENTINEL, dtype=U32) if voxel is None else np.array(voxel, dtype=U32)
    bx, bv, _, _ = births(o, field, masks, threshold, rate, max_per_voxel, seed)
    wanted = start + len(bx)
    live = min(wanted, capacity_rows)
    fit = max(0, min(len(bx), capacity_rows - start))
    out_x[start:start + fit] = bx[:fit]
    out_v[start:start + fit] = bv[:fit]
    if fill:
        out_x.view(U32)[live:] = NAN_WORD
        out_v[live:] = NO_VOXEL
    return out_x, out_v, live, wanted


def sentinels(capacity_rows):
    return np.full((capacity_rows, 3), XYZ_SENTINEL, dtype=U32).view(F), np.full(capacity_rows, VOXEL_SENTINEL, dtype=U32)


def restate_select(flags, at_least):
    """-> (slot uint32, live)"""
    keep = np.asarray(flags, dtype=np.uint8) >= at_least
    slot = np.where(keep, np.cumsum(keep) - keep, DROPPED).astype(U32)
    return slot, int(keep.sum())


def restate_compact(src, dst, flags, at_least, fill_word=None):
    """dst (rows >= n, as uint32 words) after the compact of the n = len(flags) rows of src"""
    n = len(flags)
    keep = np.asarray(flags, dtype=np.uint8) >= at_least
    out = np.array(dst).view(U32).reshape(len(dst), -1).copy()
    s = np.asarray(src).view(U32).reshape(len(src), out.shape[1])
    live = int(keep.sum())
    out[:live] = s[:n][keep]
    if fill_word is not None:
        out[live:n] = fill_word
    return out


def same_birth(got, want, what=""):
    """(xyz, voxel, live, wanted) against (xyz, voxel, live, wanted), the arrays as words"""
    assert (got[2], got[3]) == (want[2], want[3]), f"{what}: (live, wanted) {got[2:]} against {want[2:]}"
    for name, g, w in (("xyz", got[0], want[0]), ("voxel", got[1], want[1])):
        g, w = np.ascontiguousarray(g).view(U32).reshape(-1), np.ascontiguousarray(w).view(U32).reshape(-1)
        assert g.shape == w.shape, f"{what}: {name} has {g.shape} words, expected {w.shape}"
        d = np.flatnonzero(g != w)
        assert len(d) == 0, f"{what}: {name} differs in {len(d)} of {g.size} words, first at {d[:4].tolist()}: {g[d[:4]].tolist()} against {w[d[:4]].tolist()}"


# ---- fields, masks and capacities ---------------------------------------------------------------------------------------------------------------------------------------

SPEC = dict(threshold=0.25, rate=2.5, max_per_voxel=4, seed=20)  # the random fields' rule: v uniform in -0.5 .. 2 gives every count 0 .. 4
FIELDS = ("zero", "saturated", "random", "at_threshold", "masked")
FAR_SEED = 3  # SPEC's seed on sparse_far with the saturated field: a seed whose draws clamp a coordinate of the far leaves (searched on the CPU, asserted by the test)


@functools.lru_cache(maxsize=None)
def random_field(name, seed=1):
    n = len(origins(name)) * 512
    rng = np.random.default_rng([seed, GRIDS.index(name)])
    v = rng.uniform(-0.5, 2.0, n).astype(F)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def case(grid_name, kind):
    """-> (field, masks or None, spec without fill): computed once, never written"""
    o = origins(grid_name)
    n, L = len(o) * 512, len(o)
    rng = np.random.default_rng([7, GRIDS.index(grid_name), FIELDS.index(kind)])
    spec, masks = dict(SPEC), None
    if kind == "zero":
        v = np.zeros(n, dtype=F)
        spec["threshold"] = -1.0  # every voxel is eligible, and bears nothing: m = 0
    elif kind == "saturated":
        v = np.full(n, 7.0, dtype=F)
        spec.update(max_per_voxel=16, rate=3.0, seed=FAR_SEED)  # v * rate = 21 >= K
    elif kind == "random":
        v = random_field(grid_name).copy()
        special = np.array([np.nan, np.inf, -np.inf, -0.0, -3.0], dtype=F)
        at = rng.choice(n, size=min(n // 8, 200), replace=False)
        v[at] = special[np.arange(len(at)) % len(special)]
    elif kind == "at_threshold":
        v = random_field(grid_name).copy()
        v[rng.random(n) < 0.5] = F(spec["threshold"])  # exactly at the threshold: not above it
        v[::7] = np.nextafter(F(spec["threshold"]), F(np.inf))
    else:
        v = random_field(grid_name, seed=2).copy()
        bits = rng.random((L, 512)) < rng.choice([0.0, 0.1, 0.5, 1.0], size=(L, 1))
        masks = np.packbits(bits.reshape(L, 64, 8), axis=2, bitorder="little").reshape(L, 64)
        masks.setflags(write=False)
    v.setflags(write=False)
    return v, masks, spec


def capacities(c):
    """the capacity_rows cases of a field whose voxels bear c -> {name: (capacity_rows, start, fill)}"""
    wanted = int(c.sum())
    out = {"zero_rows": (0, 0, True), "exact": (wanted, 0, True), "roomy_filled": (wanted + 37, 0, True), "roomy_kept": (wanted + 37, 0, False),
           "appended": (wanted + 50, 13, True), "appended_short": (max(wanted // 2, 1) + 13, 13, True)}
    if wanted >= 2:
        out["cut_short"] = (wanted // 2, 0, True)
    runs = np.flatnonzero(c >= 2)
    if len(runs):  # a cut inside a voxel's run: its first birth fits, its second does not
        e = int(runs[len(runs) // 2])
        out["cut_inside_a_run"] = (int(c[:e].sum()) + 1, 0, False)
    return out
