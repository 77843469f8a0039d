"""TEST HELPER of tests/test_neighbours.py (CPU) and tests/test_neighbours_gpu.py: point neighbourhoods restated in numpy from the text of include/hns.h ("POINT
NEIGHBOURHOODS THROUGH A LEAF ORDER"; never from the C++), the point sets the query (hns_neighbours.hip, hns_grid_point_neighbours) is run on, and the conditions those sets
must meet -- counted by the restatement, never by the code under test.

The definition: a point takes part iff it sorts and its cell's leaf exists (its voxel key is below 512 L: order_cases.voxel_keys). h = radius. The box of point i along
axis c is the cells floorf(x_i.c - h) .. floorf(x_i.c + h), f32 operations. j is a neighbour of i iff j != i, j takes part, Floor(x_j) lies in the box on all three axes and,
with d = x_i - x_j per axis (f32), d2 = (dx*dx + dy*dy) + dz*dz, inv = 1.0f / (h*h), q = d2 * inv: q < 1.0f. Then a = 1.0f - q, w = a * a. count = the number of
neighbours; density sums rint((double)w * 2^32); push sums rint((double)(d_c * (w / sqrtf(d2))) * 2^32) over the pairs with d2 > 0; each sum a becomes
(float)((double)a * 2^-32). A point that takes no part gets count 0, density +0.0f and push +0.0f. float32 arrays: every operation below rounds once; float64 for the rint.

The two point-order entry points are operations of tests/sequence_cases.py (neighbours_original, neighbours_ranked, cell_table), whose GPU test holds one query of a
script to `restate` below. Neither call has a `void* stream` parameter, so tests/stream_cases.py needs nothing."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import order_cases as oc
import points_cases as pc

F = np.float32
GRIDS = pc.GRIDS
COUNTS = pc.COUNTS
RADII = (0.5, 0.73, 1.0, 1.5, 2.0)
N_POINTS = pc.N_POINTS
LATTICE_GRID = "dense32"
LATTICE_RADII = (0.5, 187.0 / 256.0, 1.0, 1.5, 2.0)  # multiples of 2^-8
N_LATTICE = 1500

Result = namedtuple("Result", "count density push pairs d2")  # pairs: (m, 2) original indices (i, j) of the neighbour pairs; d2: their squared distances


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------------------------------------


def takes_part(grid, n_leaves, xyz):
    return oc.voxel_keys(grid, n_leaves, xyz) < np.uint32(512 * n_leaves) if n_leaves else np.zeros(len(xyz), dtype=bool)


def box_of(x, h):
    """(lo, hi) int64 cells per axis of positions that take part: floorf(x - h), floorf(x + h)"""
    h = F(h)
    low, high = (x - h).astype(F), (x + h).astype(F)
    return np.floor(low).astype(np.int64), np.floor(high).astype(np.int64)


def finish(acc):
    return (acc.astype(np.float64) * 2.0 ** -32).astype(F)


def restate(grid, n_leaves, xyz, radius):
    """brute force over all pairs of the points that take part -> Result, rows in the order of xyz"""
    x = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n, h = len(x), F(radius)
    assert F(0) < h <= F(2)
    idx = np.flatnonzero(takes_part(grid, n_leaves, x))
    xp = x[idx]
    lo, hi = box_of(xp, h)
    cell = np.floor(xp).astype(np.int64)
    inbox = np.ones((len(idx), len(idx)), dtype=bool)
    for a in range(3):
        inbox &= (cell[None, :, a] >= lo[:, None, a]) & (cell[None, :, a] <= hi[:, None, a])
    np.fill_diagonal(inbox, False)
    I, J = np.nonzero(inbox)
    d = (xp[I] - xp[J]).astype(F)
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    xy = xx + yy
    d2 = xy + zz
    r2 = h * h
    inv = F(1.0) / r2
    q = d2 * inv
    ok = q < F(1.0)
    I, J, d, d2, q = I[ok], J[ok], d[ok], d2[ok], q[ok]
    a = F(1.0) - q
    w = a * a
    assert all(v.dtype == F for v in (d, d2, q, w, inv))
    count = np.zeros(n, dtype=np.uint32)
    count[idx] = np.bincount(I, minlength=len(idx)).astype(np.uint32)
    acc = np.zeros((len(idx), 4), dtype=np.int64)
    np.add.at(acc[:, 0], I, np.rint(w.astype(np.float64) * 2.0 ** 32).astype(np.int64))
    far = d2 > F(0)
    dist = np.sqrt(d2[far])
    s = w[far] / dist
    assert dist.dtype == F and s.dtype == F
    for c in range(3):
        t = d[far, c] * s
        np.add.at(acc[:, 1 + c], I[far], np.rint(t.astype(np.float64) * 2.0 ** 32).astype(np.int64))
    density, push = np.zeros(n, dtype=F), np.zeros((n, 3), dtype=F)
    density[idx] = finish(acc[:, 0])
    push[idx] = finish(acc[:, 1:])
    return Result(count, density, push, np.stack([idx[I], idx[J]], axis=1), d2)


def same(got, want, what=""):
    """(count, density, push) triples as bytes; the message names the first array and row that differ"""
    for name, g, w, dt in zip(("count", "density", "push"), got, want[:3], (np.uint32, F, F)):
        g, w = np.ascontiguousarray(g).view(np.uint32).reshape(-1), np.ascontiguousarray(w, dtype=dt).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, f"{what}: {name} has {g.shape} words, expected {w.shape}"
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} of {g.size} words, first at {bad[:4].tolist()}: {g[bad[:4]].tolist()} against {w[bad[:4]].tolist()}"


def cell_table(keys, n_leaves):
    """cell_start of sorted voxel keys: entry v = the number of ranks that take part whose key is < v"""
    keys = np.asarray(keys).view(np.uint32).astype(np.int64)
    inside = keys[keys < 512 * n_leaves]
    return np.searchsorted(inside, np.arange(512 * n_leaves + 1), side="left").astype(np.uint32)


# ---- the point sets -------------------------------------------------------------------------------------------------------------------------------------------------------


def corner_of_eight(o):
    """a corner where eight leaves of the set meet, or None"""
    have = set(map(tuple, np.asarray(o).tolist()))
    for q in sorted(have):
        if all((q[0] - 8 * (c >> 2), q[1] - 8 * ((c >> 1) & 1), q[2] - 8 * (c & 1)) in have for c in range(8)):
            return np.array(q, dtype=np.float64)
    return None


def _ball(rng, centre, n, radius):
    d = rng.standard_normal((n, 3))
    d *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return np.asarray(centre, dtype=np.float64) + d


def _crafted(o, rng):
    """the points that carry the conditions, from the leaf origins alone"""
    o = np.asarray(o, dtype=np.int64)
    parts = []
    hub = corner_of_eight(o)
    site = hub if hub is not None else o[len(o) // 2].astype(np.float64) + 4.0
    parts.append(_ball(rng, site, 150, 1.9))                                                        # (a), (i): eight leaves under one ball, or the middle of a leaf
    parts.append(site + np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3))  # (e): integer coordinates, leaf faces among them
    faces = pc.absent_faces(o)
    for f in range(3):                                                                              # (b), (c): either side of a face whose neighbour is absent
        org, axis, sign = faces[(f * 7919) % len(faces)]
        c = np.asarray(org, dtype=np.float64) + rng.uniform(2.0, 6.0, 3)
        c[axis] = org[axis] + (8.0 if sign > 0 else 0.0)
        parts.append(_ball(rng, c, 60, 1.8))
    first = o[0].astype(np.float64)
    heavy = first + np.array([1.0, 2.0, 3.0]) + rng.uniform(0.01, 0.99, (300, 3))                    # (f): 300 points in one voxel
    parts.append(heavy)
    parts.append(first + np.array([5.0, 6.0, 1.0]) + rng.uniform(0.01, 0.99, (65, 3)))              # (f): exactly 65 in another
    parts.append(np.concatenate([parts[0][:20], heavy[:10], parts[1][:10]]))                        # (d): coincident pairs
    parts.append(np.nextafter((site + np.array([[0.0, 1.0, 0.5], [8.0, 0.25, 0.0]])).astype(F), F(-np.inf)).astype(np.float64))  # an ulp below an integer: x + h rounds up
    special = np.tile(site, (12, 1))                                                               # (g): rows that take no part, next to points that do
    special[0, 0] = special[1, 1] = special[2, 2] = np.nan
    special[3, 0], special[4, 1], special[5] = np.inf, -np.inf, np.nan
    special[6, 2], special[7, 0], special[8, 1] = 2.0 ** 23, -(2.0 ** 23), 2.0 ** 23 - 1.0
    special[9], special[10] = np.inf, -np.inf
    special[11] = [2.0 ** 23, 2.0 ** 23, 2.0 ** 23]
    parts.append(special)
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def full_set(name):
    """N_POINTS points on the grid: the crafted ones and points_cases.make_points for the rest, in one fixed shuffle; computed once, never written"""
    o = oc.origins(name)
    rng = np.random.default_rng([GRIDS.index(name), 53])
    with np.errstate(invalid="ignore"):
        crafted = _crafted(o, rng).astype(F)
    rest = pc.make_points(o, 100 + GRIDS.index(name), N_POINTS - len(crafted))
    xyz = np.concatenate([crafted, rest])[rng.permutation(N_POINTS)]
    # the voxel of 65 holds no other point: one that strayed into it moves a leaf's width away along x, out of the leaf
    v65 = np.asarray(o[0], dtype=np.float64) + np.array([5.0, 6.0, 1.0])
    keep = np.zeros(N_POINTS, dtype=bool)
    with np.errstate(invalid="ignore"):
        inside = (np.floor(xyz) == v65.astype(F)).all(1)
    keep[np.flatnonzero(inside)[:65]] = True
    xyz[inside & ~keep, 0] += F(8.0)
    xyz = np.ascontiguousarray(xyz, dtype=F)
    xyz.setflags(write=False)
    return xyz


def points(name, count):
    return full_set(name)[:count]


@functools.lru_cache(maxsize=None)
def expected(name, count, radius):
    """the restatement on a prefix of the grid's set: computed once, shared, never written"""
    r = restate(oc.host_grid(name), len(oc.origins(name)), points(name, count), radius)
    for a in r:
        a.setflags(write=False)
    return r


def leaf_of(xyz):
    return np.floor(np.asarray(xyz, dtype=np.float64)).astype(np.int64) & ~7


def conditions(name, radius=2.0):
    """what the grid's full set carries at `radius`, counted on the restatement -> dict"""
    o = oc.origins(name)
    g, L = oc.host_grid(name), len(o)
    x = full_set(name)
    r = expected(name, N_POINTS, radius)
    part = takes_part(g, L, x)
    key = oc.voxel_keys(g, L, x)
    out = {}
    # (a) neighbour pairs across a face, an edge and a corner: the leaves of the two points differ along 1, 2, 3 axes
    li, lj = leaf_of(x[r.pairs[:, 0]]), leaf_of(x[r.pairs[:, 1]])
    axes = (li != lj).sum(1)
    out["face"], out["edge"], out["corner"] = (int((axes == k).sum()) for k in (1, 2, 3))
    # (b) points that take part whose box reaches into an absent leaf: one of the box's eight corner cells has no leaf
    idx = np.flatnonzero(part)
    lo, hi = box_of(x[idx], radius)
    absent = np.zeros(len(idx), dtype=bool)
    for c in range(8):
        corner = np.where(np.array([c >> 2, (c >> 1) & 1, c & 1], dtype=bool), hi, lo).astype(np.int32)
        absent |= g.offsets(corner) == 0
    out["box_into_absent_leaf"] = int(absent.sum())
    # (c) sorting points outside every leaf within h of a point that takes part (float64 distances: a count, not the arithmetic under test)
    outside = np.flatnonzero(key == np.uint32(512 * L))
    near = 0
    xi = x[idx].astype(np.float64)
    for p in outside:
        near += bool((((xi - x[p].astype(np.float64)) ** 2).sum(1) < float(radius) ** 2).any())
    out["outside_within_h"] = near
    out["outside_unrelated"] = bool((r.count[~part] == 0).all() and not r.density[~part].view(np.uint32).any() and not r.push[~part].view(np.uint32).any()
                                    and not np.isin(r.pairs, np.flatnonzero(~part)).any())
    # (d) coincident pairs
    out["coincident_pairs"] = int((r.d2 == 0).sum())
    # (e) points that take part on integer coordinates, and on leaf faces
    xp = x[idx]
    out["integer"] = int((xp == np.floor(xp)).any(1).sum())
    out["on_leaf_face"] = int(((xp == np.floor(xp)) & (np.floor(xp).astype(np.int64) % 8 == 0)).any(1).sum())
    # (f) the fullest voxel, and voxels of exactly 65
    per_voxel = np.bincount(key[part].astype(np.int64), minlength=512 * L)
    out["fullest_voxel"], out["voxels_of_65"] = int(per_voxel.max()), int((per_voxel == 65).sum())
    # (g) rows that take no part
    out["nan_rows"], out["plus_inf_rows"], out["minus_inf_rows"] = int(np.isnan(x).any(1).sum()), int((x == np.inf).any(1).sum()), int((x == -np.inf).any(1).sum())
    out["rows_at_2^23"] = int((np.abs(x) == F(2.0 ** 23)).any(1).sum())
    # (i) the most leaves one point's neighbours lie in
    most = 0
    if len(r.pairs):
        lid = np.unique(lj, axis=0, return_inverse=True)[1].reshape(-1)
        pairs = np.unique(np.stack([r.pairs[:, 0], lid], axis=1), axis=0)
        most = int(np.bincount(pairs[:, 0]).max())
    out["leaves_of_one_points_neighbours"] = most
    out["six_cell_boxes"] = int(((hi - lo + 1) == 6).any(1).sum())
    return out


def empty_leaf_between_populated(name, count):
    """(h): the number of leaves that hold no point of the prefix while both neighbours along some axis exist and hold one"""
    o = np.asarray(oc.origins(name), dtype=np.int64)
    g, L = oc.host_grid(name), len(o)
    x = points(name, count)
    key = oc.voxel_keys(g, L, x)
    per_leaf = np.bincount((key[key < 512 * L] >> 9).astype(np.int64), minlength=L)
    ids = {tuple(q): i for i, q in enumerate(o.tolist())}
    found = 0
    for q, i in ids.items():
        if per_leaf[i]:
            continue
        for axis in range(3):
            a, b = list(q), list(q)
            a[axis] -= 8
            b[axis] += 8
            if tuple(a) in ids and tuple(b) in ids and per_leaf[ids[tuple(a)]] and per_leaf[ids[tuple(b)]]:
                found += 1
                break
    return found


# ---- the lattice set: coordinates and radii that are multiples of 2^-8 in a 32^3 box --------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def lattice_set():
    """N_LATTICE points on multiples of 2^-8 strictly inside the 32^3 box of LATTICE_GRID, in thirty clumps. There every difference is exact, every square and sum below
    (h + 1)^2 is exact (10-bit differences: 20-bit squares, 22-bit sums), and x +- h is exact, so |d_c| <= h puts Floor(x_j) into i's box: the box never cuts a pair the
    weight accepts, the pair relation is symmetric, and a reflection through the centre keeps every |d|."""
    rng = np.random.default_rng(2024)
    centres = rng.uniform(3.0, 29.0, (30, 3))
    x = centres[rng.integers(0, 30, N_LATTICE)] + rng.uniform(-1.25, 1.25, (N_LATTICE, 3))
    a = np.clip(np.rint(x * 256.0), 1, 32 * 256 - 1)
    a[:40] = np.rint(a[:40] / 256.0) * 256.0  # integer coordinates among them
    a = np.clip(a, 256, 31 * 256)
    a[40:60] = a[:20]  # coincident pairs
    xyz = np.ascontiguousarray((a / 256.0).astype(F))
    assert (xyz.astype(np.float64) * 256.0 == a).all() and (xyz > 0).all() and (xyz < 32).all()
    xyz.setflags(write=False)
    return xyz


def reflected(xyz):
    """through the centre of the 32^3 box; LATTICE_GRID's leaves reflect onto themselves"""
    return np.ascontiguousarray((F(32.0) - np.asarray(xyz, dtype=F)).astype(F))


def negated_push(push):
    """-push in every bit; an empty sum is +0.0f on both sides"""
    p = np.asarray(push, dtype=F)
    return np.where(p == 0, p, -p).astype(F)
