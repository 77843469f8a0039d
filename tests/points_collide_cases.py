"""TEST HELPER of tests/test_points_collide_cases.py (CPU) and tests/test_points_collide_gpu.py: the collision SDFs that points are traced against, and the mirror of
k_trace_points_collide (hns_points_collide.hip) restated from the text of include/hns.h: numpy float32, one rounded operation per line, with S(x) the oracle's
sample_trilinear_f, U(x) its sample_trilinear_v on the fmaf branch of the Vec3f lerp and RK(x) one step of points_cases.trace_mirror. Nothing here calls the library under
test: the mirror is the oracle of every comparison, and the classes the conditions count are its own.

The SDF is a lattice of spheres of radius 3 voxels centred on every leaf corner, in closed form over a voxel's coordinates c: m = ((c + 4) mod 8) - 4,
sdf = float32((sqrt(float64(m . m)) - 3) / 24) -- world units at 24 voxels per unit, as points_cases.INV_DX has it. Every surface crosses leaf faces (a sphere lies in the
eight leaves around its corner), and 22 % of the volume is inside. The banded variant holds the reference's fill value (bytes 01 01 01 01, 2.4e-38) wherever
|sdf| > 2 / 24: what a narrow-band level set looks like once it is copied onto the domain."""
from __future__ import annotations

import functools

import numpy as np

import points_cases as pc
import special_cases as sc
from oracle_lib import OracleGrid

F = np.float32
MODES = ("stop", "push", "kill")
VARIANTS = ("full", "banded")
HIT_PUSHED, HIT_REVERTED, HIT_KILLED, HIT_START = 1, 2, 4, 8
THRESHOLD, SKIN, ITERATIONS = 0.0, 1.0 / 16, 3  # of the conditions and of the GPU comparison


def lattice_sdf(coords, variant="full"):
    c = np.asarray(coords, dtype=np.int64)
    m = ((c + 4) % 8) - 4
    sdf = ((np.sqrt((m * m).sum(1).astype(np.float64)) - 3.0) / 24.0).astype(F)
    if variant == "banded":
        sdf = np.where(np.abs(sdf) > F(2.0 / 24.0), sc.SDF_FILL, sdf).astype(F)
    return np.ascontiguousarray(sdf)


@functools.lru_cache(maxsize=None)
def sdf_of(name, variant):
    """the SDF of a grid of points_cases.GRIDS: computed once, never written"""
    s = lattice_sdf(OracleGrid(pc.case(name)[0]).coords(), variant)
    s.setflags(write=False)
    return s


def normal(nb, inv_dx):
    """sdf_normal_of (hns_device.hpp) restated: nb = six arrays in the order -x, +x, -y, +y, -z, +z -> [n, 3]"""
    s = F(0.5) * F(inv_dx)
    g = []
    for a in range(3):
        diff = nb[2 * a + 1] - nb[2 * a]
        g.append(s * diff)
    xx = g[0] * g[0]
    yy = g[1] * g[1]
    zz = g[2] * g[2]
    t = xx + yy
    t = t + zz
    length = np.sqrt(t)
    ok = length > F(1e-6)  # (a NaN length: no)
    inv = F(1.0) / length
    return np.stack([np.where(ok, inv * c, F(0.0)) for c in g], axis=1).astype(F)


def push_out(S, x1, d, coll, thr, skin, inv, iterations, on_first=None):
    """push_out (hns_pointstep.hpp) restated, in place on x1 [m, 3] and d = S(x1): the rows of `coll` are pushed while d < thr, at most `iterations` times.
    on_first(idx, nrm): what the caller does with the first iteration's rows and normals. -> per-row counts (first_push, later_push, inside): steps the first / a later
    push resolved, and steps still inside after the last"""
    one = F(1.0)
    first_push, later_push, inside = (np.zeros(len(x1), np.int64) for _ in range(3))
    for it in range(iterations):
        idx = np.flatnonzero(coll & (d < thr))
        if not len(idx):
            break
        p, nb = x1[idx], []
        for axis in range(3):
            for sign in (-1, 1):
                q = p.copy()
                q[:, axis] = p[:, axis] - one if sign < 0 else p[:, axis] + one
                nb.append(S(q))
        nrm = normal(nb, inv)
        if it == 0 and on_first is not None:
            on_first(idx, nrm)
        a = thr - d[idx]
        a = a * inv
        a = a + skin
        move = a[:, None] * nrm
        p = p + move
        x1[idx] = p
        d[idx] = S(p)
        out = idx[~(d[idx] < thr)]
        (first_push if it == 0 else later_push)[out] += 1
    inside[coll & (d < thr)] += 1
    return first_push, later_push, inside


def collide_mirror(G: OracleGrid, vel, sdf, xyz, dt, inv_dx, order, steps, mode, threshold=THRESHOLD, skin=SKIN, iterations=ITERATIONS):
    """-> (final positions [n, 3], status bytes, hit bytes, classes): classes is a dict of per-point counts of STEPS -- first_push / later_push: steps the first / a
    later push resolved; push_reverted: steps put back after the last push"""
    assert mode in MODES
    thr, skin, inv = F(threshold), F(skin), F(inv_dx)
    x = np.array(xyz, dtype=F)
    n = len(x)
    S = lambda q: G.sample_trilinear_f(sdf, np.ascontiguousarray(q, dtype=F)) if len(q) else np.zeros(0, F)
    hit = np.zeros(n, np.uint8)
    dead = np.zeros(n, bool)
    first_push, later_push, push_reverted = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        hit[S(x) < thr] |= HIT_START
        for _ in range(steps):
            x0 = x
            x1 = np.array(pc.trace_mirror(G, vel, x0, dt, inv_dx, order, 1)[0][-1], dtype=F)  # RK(x0): one step, its operations
            d = S(x1)
            coll = (d < thr) & ~dead
            if mode == "stop":
                hit[coll] |= HIT_REVERTED
                x1[coll] = x0[coll]
            elif mode == "kill":
                hit[coll] |= HIT_KILLED
            else:
                hit[coll] |= HIT_PUSHED
                first, later, inside = push_out(S, x1, d, coll, thr, skin, inv, iterations)
                first_push += first
                later_push += later
                push_reverted += inside
                rev = inside > 0
                hit[rev] |= HIT_REVERTED
                x1[rev] = x0[rev]
            x = np.where(dead[:, None], x0, x1).astype(F)  # (a dead point takes no further step)
            if mode == "kill":
                dead |= coll
    status = (~dead & np.isfinite(x).all(1) & pc.leaf_exists(G, x)).astype(np.uint8)
    return x, status, hit, {"first_push": first_push, "later_push": later_push, "push_reverted": push_reverted}


def leaf_of(xyz):
    return np.floor(np.asarray(xyz, dtype=np.float64) / 8.0)


def classes(xyz, got, hit, cls):
    """the counts the conditions of tests/test_points_collide_cases.py are stated on: points, but for the three outcomes of a pushed step, which are steps"""
    pushed = (hit & HIT_PUSHED) != 0
    return {"start_in": int(((hit & HIT_START) != 0).sum()), "never_hit": int((hit == 0).sum()), "reverted": int(((hit & HIT_REVERTED) != 0).sum()),
            "killed": int(((hit & HIT_KILLED) != 0).sum()), "first_push": int(cls["first_push"].sum()), "later_push": int(cls["later_push"].sum()), "push_reverted": int(cls["push_reverted"].sum()),
            "pushed_other_leaf": int((pushed & (leaf_of(got) != leaf_of(xyz)).any(1)).sum())}
