"""TEST HELPER of tests/test_splat.py (CPU) and tests/test_splat_gpu.py: point values added into fields (hns_dev_splat_points, its host mirror hns_grid_splat_points).

`restate` is the arithmetic of include/hns.h written again in numpy from the header's text alone: float32 arrays so that every operation rounds once, Floor and the cell
by points_cases.cell_of, leaf lookup through the ORACLE's grid, the sum by np.add.at on int64 (which wraps modulo 2^64 as the accumulators do). The host mirror is held to it
in every byte on the CPU; the device is held to the host mirror on the GPU.

`case(name)` is a grid's fields, points and point values. Its points are points_cases.make_points' 4,099 with 80 more inside ONE cell (the contended voxels), mixed, and the
conditions the issue sets are asserted here, on the CPU, from the restatement alone:
  status classes   points with no tap landed, with some (1 .. 7) and with all 8, each class non-empty
  crossing         some landed cell has its lower corner on local index 7 along exactly one, exactly two and all three axes
  negative         some position component is negative
  integral         some landed point sits exactly on a voxel
  contention       at least one voxel receives 64 terms or more
"""
from __future__ import annotations

import functools

import numpy as np

import points_cases as pc
from frame_cases import random_masks
from oracle_lib import OracleGrid

F = np.float32
GRIDS = pc.GRIDS
COUNTS = pc.COUNTS
QUANTA = (-40, -32, -8)
N_CLUSTER = 80


def wrap32(a):
    """int64 -> the int32 of the same low 32 bits (corner coordinates wrap at the end of the range, as the device's unsigned adds do)"""
    return ((np.asarray(a, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)


def voxel_of(G: OracleGrid, ijk):
    """flat voxel index of each coordinate by the oracle's lookup, -1 where its leaf is absent"""
    assert G.N < 2 ** 24  # the index travels through a float32 field
    ok = (np.abs(ijk) < 2 ** 31 - 16).all(1)  # (no leaf of a test grid lies out there; the oracle's own arithmetic is kept away from the end of the range)
    number = np.arange(1, G.N + 1, dtype=F)
    got = G.sample_nearest_f(number, np.where(ok[:, None], ijk, 0).astype(np.int32)).astype(np.int64)
    return np.where(ok, got, 0) - 1


def cell_taps(G: OracleGrid, xyz):
    """-> (idx [n, 8] flat voxel of tap di*4+dj*2+dk or -1, w [n, 8] float32 weights, ijk): the header's Cell, Weights and Landing"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    finite = np.isfinite(xyz).all(1)
    ijk = pc.cell_of(xyz)
    with np.errstate(all="ignore"):
        f = xyz - ijk.astype(F)
        one = F(1.0)
        wx, wy, wz = [one - f[:, 0], f[:, 0]], [one - f[:, 1], f[:, 1]], [one - f[:, 2], f[:, 2]]
        idx, w = np.full((n, 8), -1, dtype=np.int64), np.zeros((n, 8), dtype=F)
        for c in range(8):
            di, dj, dk = c >> 2, (c >> 1) & 1, c & 1
            w[:, c] = (wx[di] * wy[dj]) * wz[dk]
            corner = wrap32(ijk.astype(np.int64) + np.array([di, dj, dk]))
            idx[:, c] = np.where(finite, voxel_of(G, corner), -1) if n else -1
    assert w.dtype == F
    return idx, w, ijk


def restate(G: OracleGrid, fields, xyz, values, log2_quantum, masks=None, activate=True):
    """The header's text in numpy. fields: (N,) / (N, 3) float32 arrays (not written); -> (new fields, status, rejected, new masks or None, accepted k of every
    channel as a list of int64 arrays)"""
    idx, w, _ = cell_taps(G, xyz)
    landed = idx >= 0
    status = landed.sum(1).astype(np.uint8)
    new_masks = None
    if masks is not None:
        new_masks = np.array(masks, dtype=np.uint8).reshape(-1)
        if activate:
            with np.errstate(invalid="ignore"):
                on = landed & (w > 0)
            np.bitwise_or.at(new_masks, idx[on] >> 3, (1 << (idx[on] & 7)).astype(np.uint8))
        new_masks = new_masks.reshape(np.asarray(masks).shape)
    scale, quantum = 2.0 ** (-log2_quantum), 2.0 ** log2_quantum
    out, rejected, ks = [], 0, []
    for field, vals in zip(fields, values):
        new = np.array(field, dtype=F)
        ncomp = new.size // G.N
        flat, v = new.reshape(G.N, ncomp), np.asarray(vals, dtype=F).reshape(len(idx), ncomp)
        for comp in range(ncomp):
            with np.errstate(all="ignore"):
                t = w * v[:, comp][:, None]
                assert t.dtype == F
                x = t.astype(np.float64) * scale
                accepted = landed & (np.abs(x) < 2.0 ** 62)  # (a NaN and an inf fail the comparison)
            rejected += int((landed & ~accepted).sum())
            k = np.rint(x[accepted]).astype(np.int64)
            ks.append(k)
            acc = np.zeros(G.N, dtype=np.int64)
            np.add.at(acc, idx[accepted], k)
            nz = np.flatnonzero(acc)
            with np.errstate(all="ignore"):
                flat[nz, comp] = flat[nz, comp] + (acc[nz].astype(np.float64) * quantum).astype(F)
        out.append(new)
    return out, status, rejected, new_masks, ks


def check_conditions(G: OracleGrid, xyz, name):
    idx, w, ijk = cell_taps(G, xyz)
    status = (idx >= 0).sum(1)
    assert (status == 0).any() and ((status > 0) & (status < 8)).any() and (status == 8).any(), f"{name}: status classes {np.bincount(status, minlength=9).tolist()}"
    on7 = ((ijk & 7) == 7).sum(1)[status > 0]
    assert all((on7 == a).any() for a in (1, 2, 3)), f"{name}: landed cells with the lower corner on local index 7 along 0..3 axes: {np.bincount(on7, minlength=4).tolist()}"
    assert (xyz < 0).any(), f"{name}: no negative position"
    integral = (xyz == np.floor(xyz)).all(1) & np.isfinite(xyz).all(1)
    assert (integral & (idx[:, 0] >= 0)).any(), f"{name}: no landed point exactly on a voxel"
    terms = np.bincount(idx[idx >= 0], minlength=G.N)
    assert terms.max() >= 64, f"{name}: the busiest voxel receives {terms.max()} terms"


@functools.lru_cache(maxsize=None)
def case(name):
    """(origins, velocity, float fields with -0.0 planted, points, point values per float field, point values of the velocity, active masks): computed once, never written"""
    o, vel, phi, xyz = pc.case(name)
    rng = np.random.default_rng([61, GRIDS.index(name)])
    cell = o[0].astype(np.float64) + np.array([2.0, 3.0, 4.0])
    cluster = (cell + rng.uniform(0.05, 0.95, (N_CLUSTER, 3))).astype(F)
    pts = np.concatenate([xyz, cluster])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    vel, phi = np.array(vel), [np.array(p) for p in phi[:6]]
    for a in [vel, *phi]:
        a[rng.random(a.shape) < 0.05] = -0.0  # an untouched voxel keeps the sign
    vals = [(rng.standard_normal(len(pts)) * 3.0).astype(F) for _ in phi]
    vvals = (rng.standard_normal((len(pts), 3)) * 3.0).astype(F)
    masks = random_masks(GRIDS.index(name) + 7, len(o))
    for a in [vel, pts, vvals, masks, *phi, *vals]:
        a.setflags(write=False)
    return o, vel, phi, pts, vals, vvals, masks


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    G = OracleGrid(case(name)[0])
    check_conditions(G, case(name)[3], name)
    return G


def host_grid(origins, vs=1.0 / 24.0):
    from hnanosolver_amd import _lib, api

    return api.create_grid_from_leaves(origins, vs, _lib.HNS_GRID_HOST_ONLY)


def mirror(grid, fields, xyz, values, log2_quantum=-32, masks=None, activate=True):
    """the host mirror on copies -> (new fields, status, rejected, new masks or None)"""
    from hnanosolver_amd import api

    new = [np.array(f, dtype=F) for f in fields]
    m = None if masks is None else np.array(masks, dtype=np.uint8)
    status = np.full(len(xyz), 0xAB, dtype=np.uint8)
    rejected = api.splat_points_host(grid, new, xyz, values, log2_quantum, m, activate, status)
    return new, status, rejected, m


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def channel_sets(name):
    """{set name: (fields, point values)} of the issue's channel sets: float alone, Vec3f alone, 1 float + velocity (4 channels, one launch), 5 floats + velocity (8 channels)"""
    _, vel, phi, _, vals, vvals, _ = case(name)
    return {
        "float": ([phi[0]], [vals[0]]),
        "vec3": ([vel], [vvals]),
        "float+vec3": ([phi[1], vel], [vals[1], vvals]),
        "5float+vec3": (phi[:5] + [vel], vals[:5] + [vvals]),
    }
