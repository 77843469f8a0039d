"""TEST HELPER of the diagnostics tests (tests/test_diagnostics.py, tests/test_diagnostics_gpu.py, tests/test_pool_contents_gpu.py): numpy restatements of the two
things include/hns.h defines bit for bit -- the reduction behind an hns_stats record and the Gauss-Seidel correction c of the pressure residual -- written from the
header's text, not from the library's code; and, for the GPU tests, the comparisons of the device diagnostics with them and with leafio.leaf_stats."""
import math

import numpy as np

import special_cases as sc
from frame_cases import assert_same, download
from hnanosolver_amd import _lib, api, device as D, leafio
from hnanosolver_amd._lib import lib

F = np.float32
INV6 = F(0.166666667)
DX = 0.1
REL, EVERY = 1e-3, 4  # the controlled solve of the GPU tests: relative tolerance, iterations between two checks
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


# ---------------------------------------------------------------------------------------------------------------
# on the GPU (torch is imported where it is used: this module also serves the tests that run without one)
# ---------------------------------------------------------------------------------------------------------------


def leaf_ids(n):
    import torch

    return torch.arange(n, dtype=torch.int32, device="cuda")


def read_field(ptr, n_leaves):
    """a float field at a raw device pointer of the library, through the library's own whole-leaf copy"""
    import torch

    out = torch.empty(n_leaves * 512, dtype=torch.float32, device="cuda")
    D._raise(lib.hns_dev_pack_leaves(ptr, leaf_ids(n_leaves).data_ptr(), n_leaves, out.data_ptr(), 1, D.current_stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def write_field(ptr, values):
    import torch

    v = torch.from_numpy(np.ascontiguousarray(values, dtype=F)).cuda()
    n = v.numel() // 512
    D._raise(lib.hns_dev_unpack_leaves(v.data_ptr(), leaf_ids(n).data_ptr(), n, ptr, 1, D.current_stream()))
    torch.cuda.synchronize()


def pressure_of(sim):
    return read_field(lib.hns_sim_pressure_ptr(sim._ptr), sim.grid.leaf_count())


def set_divergence(sim, div):
    write_field(lib.hns_sim_divergence_ptr(sim._ptr), div)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).tobytes()


def special_state(seed, n, names):
    """normal values with a different special-value class planted in each field (NaN and +-inf, subnormals, signed zeros, 3e37, ...)"""
    rng = np.random.default_rng(seed)
    st = {"vel": sc.plant("nonfinite", rng.standard_normal((n * 512, 3)).astype(F), rng)}
    for i, k in enumerate(names):
        st[k] = sc.plant(sc.CLASSES[i % len(sc.CLASSES)], rng.standard_normal(n * 512).astype(F), rng)
    return st


def host_stats(sim, names, masked):
    st = download(sim, names)
    m = sim.active_masks() if masked else None
    return np.concatenate([leafio.leaf_stats(st[k], m) for k in names] + [leafio.leaf_stats(st["vel"], m)]), st


def assert_stats(sim, names, masked, what):
    want, before = host_stats(sim, names, masked)
    masks_before, ahead_before = sim.active_masks(), sim.lookahead_counts()
    got = sim.stats(names, velocity=True, masks=masked)
    assert got.tobytes() == want.tobytes(), f"{what}: {got} vs {want}"
    assert sim.stats(names, velocity=True, masks=masked).tobytes() == got.tobytes(), f"{what}: two calls differ"
    assert_same(download(sim, names), before, f"{what}: fields after stats")
    assert np.array_equal(sim.active_masks(), masks_before) and sim.lookahead_counts() == ahead_before
    return got


def check_residual(grid, o, div, p, first, count, what):
    import torch

    c_out = torch.full((len(o) * 512,), 7.0, dtype=torch.float32, device="cuda")
    rec = D.read_stats(D.residual(grid, div, p, DX, c_out))
    want = residual_numpy(o, div.cpu().numpy(), p.cpu().numpy(), DX)
    got = c_out.cpu().numpy()
    lo, hi = first * 512, (first + count) * 512
    assert sc.same_bits(got[lo:hi], want[lo:hi]), f"{what}: {sc.describe(got[lo:hi], want[lo:hi])}"
    assert (got[:lo] == 7.0).all() and (got[hi:] == 7.0).all(), f"{what}: wrote outside the launch range"
    assert rec.tobytes() == leafio.leaf_stats(got[lo:hi]).tobytes(), f"{what}: record {rec} vs {leafio.leaf_stats(got[lo:hi])}"
    assert D.read_stats(D.residual(grid, div, p, DX)).tobytes() == rec.tobytes(), f"{what}: without c_out / second call"
    return rec


def crossed(rec, initial, rel=REL, abs_tol=0.0):
    return rec["nan_count"] == 0 and rec["max_abs"] <= max(F(abs_tol), F(rel) * initial["max_abs"])


def controlled_solve_against_plain_solves(a, b, o, div, dx, maxit):
    """sims a and b on one grid with the divergence `div` set: the controlled pressure solve on a (REL, every EVERY iterations, at most maxit) against plain solves of
    EVERY, 2 EVERY, ... iterations on b -- the initial record against the numpy restatement, the stop at the first crossing (or the maximum), every history entry, the
    final record and the pressure bits. -> (report, iteration of the first crossing or None, the plain solves' records, the initial record)"""
    initial = leafio.leaf_stats(residual_numpy(o, div, np.zeros_like(div), dx))[0]
    a.solve_control(REL, 0.0, EVERY)
    a.pressure_solve(maxit, dx)
    rep = a.solve_report()
    assert rep["initial"].tobytes() == initial.tobytes()
    # the expected stop, derived from plain solves of 4, 8, ... iterations on the second sim
    stop, plain = None, []
    for j in range(EVERY, maxit + 1, EVERY):
        b.pressure_solve(j, dx)
        plain.append(b.residual(dx)[0])
        if crossed(plain[-1], initial):
            stop = j
            break
    ran = stop if stop is not None else EVERY * len(plain)
    assert rep["iterations"] == ran and bool(rep["converged"]) == (stop is not None) and rep["checks"] == ran // EVERY == len(rep["history"])
    for i, h in enumerate(rep["history"]):
        assert h.tobytes() == plain[i].tobytes(), f"history[{i}] differs from the plain solve of {EVERY * (i + 1)} iterations"
    assert rep["final"].tobytes() == plain[-1].tobytes()
    assert words(pressure_of(a)) == words(pressure_of(b))
    assert a.residual(dx)[0].tobytes() == rep["final"].tobytes()
    return rep, stop, plain, initial
