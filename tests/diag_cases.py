"""TEST HELPER of the diagnostics tests (tests/test_diagnostics.py, tests/test_diagnostics_gpu.py): numpy restatements of the two things include/hns.h
defines bit for bit -- the reduction behind an hns_stats record and the Gauss-Seidel correction c of the pressure residual -- written from the header's
text, not from the library's code."""
import math

import numpy as np

from hnanosolver_amd import _lib, api, leafio

F = np.float32
INV6 = F(0.166666667)
QNAN64 = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]


def unpack(masks, n):
    """(n, 64) mask bytes (byte x*8+y, bit z) or None -> (n, 512) bool"""
    if masks is None:
        return np.ones((n, 512), dtype=bool)
    return np.unpackbits(np.asarray(masks, dtype=np.uint8).reshape(n, 64, 1), axis=2, bitorder="little").reshape(n, 512).astype(bool)


def tree_depth(n_leaves):
    """additions on the longest path of the stated tree: 7 per lane, 6 butterfly steps, the levels over leaves"""
    return 7 + 6 + (math.ceil(math.log2(n_leaves)) if n_leaves > 1 else 0)


def tree_sum(terms):
    """terms: (n_leaves, 512) float64 -> their sum in the order include/hns.h states"""
    n = len(terms)
    if n == 0:
        return np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = terms.reshape(n, 8, 64)  # [leaf, k, lane]: voxel 64k + lane
        acc = t[:, 0, :].copy()
        for k in range(1, 8):
            acc = acc + t[:, k, :]
        m = 1
        while m < 64:  # the xor butterfly as the balanced tree over lane index
            acc[:, ::2 * m] = acc[:, ::2 * m] + acc[:, m::2 * m]
            m *= 2
        a = acc[:, 0].copy()
        s = 1
        while s < n:  # the balanced tree over leaf index, padded with +0.0
            idx = np.arange(0, n, 2 * s)
            right = np.where(idx + s < n, a[np.minimum(idx + s, n - 1)], np.float64(0.0))
            a[idx] = a[idx] + right
            s *= 2
    return QNAN64 if np.isnan(a[0]) else a[0]


def _key(x):
    b = np.asarray(x, dtype=F).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _unkey(k):
    k = np.uint32(k)
    b = k ^ (np.uint32(0x80000000) if k >> 31 else np.uint32(0xFFFFFFFF))
    return np.frombuffer(np.uint32(b).tobytes(), F)[0]


def numpy_stats(values, masks=None):
    """one component: values (n_leaves * 512,) float32, masks (n, 64) bytes or None -> (record as STATS_DTYPE[()] , terms of sum, terms of sum_sq)"""
    v = np.ascontiguousarray(values, dtype=F).reshape(-1, 512)
    n = len(v)
    on = unpack(masks, n)
    nan = np.isnan(v)
    use = on & ~nan
    r = np.zeros((), dtype=leafio.STATS_DTYPE)
    r["count"], r["nan_count"] = on.sum(), (on & nan).sum()
    keys = _key(v)[use]
    r["min"] = _unkey(keys.min()) if keys.size else F(np.inf)
    r["max"] = _unkey(keys.max()) if keys.size else F(-np.inf)
    r["max_abs"] = np.abs(v[use]).max() if keys.size else F(0.0)
    t = np.where(use, v.astype(np.float64), np.float64(0.0))
    with np.errstate(over="ignore"):
        t2 = t * t
    r["sum"], r["sum_sq"] = tree_sum(t), tree_sum(t2)
    return r, t, t2


def residual_numpy(origins, div, p, dx):
    """c = ((pxp + pxm + pyp + pym + pzp + pzm) - div * dx*dx) * 0.166666667f - p in float32 over every voxel of every leaf, absent neighbours 0"""
    origins = np.ascontiguousarray(origins, dtype=np.int32)
    n = len(origins)
    nb = api.create_grid_from_leaves(origins, float(dx), _lib.HNS_GRID_HOST_ONLY).neighbor_table()
    P = np.ascontiguousarray(p, dtype=F).reshape(n, 8, 8, 8)

    def shifted(axis, d):
        out = np.zeros_like(P)
        inner_dst, inner_src, face_dst, face_src = ([slice(None)] * 4 for _ in range(4))
        inner_dst[axis + 1], inner_src[axis + 1] = (slice(0, 7), slice(1, 8)) if d > 0 else (slice(1, 8), slice(0, 7))
        face_dst[axis + 1], face_src[axis + 1] = (7, 0) if d > 0 else (0, 7)
        out[tuple(inner_dst)] = P[tuple(inner_src)]
        leaf = nb[:, 13 + d * (9, 3, 1)[axis]]
        layer = P[np.where(leaf >= 0, leaf, 0)][tuple(face_src)].copy()
        layer[leaf < 0] = F(0.0)
        out[tuple(face_dst)] = layer
        return out

    dx2 = F(dx) * F(dx)
    d = np.ascontiguousarray(div, dtype=F).reshape(n, 8, 8, 8)
    with np.errstate(all="ignore"):
        s = shifted(0, 1) + shifted(0, -1) + shifted(1, 1) + shifted(1, -1) + shifted(2, 1) + shifted(2, -1)  # left to right, as written
        c = (s - d * dx2) * INV6 - P
    assert c.dtype == F
    return c.reshape(-1)

