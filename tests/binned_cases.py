"""TEST HELPER of tests/test_splat_binned.py (CPU) and tests/test_splat_binned_gpu.py: point values added into fields through a leaf order (hns_point_order_splat,
hns_splat_binned.hip). The ordered call promises the bytes of the plain one, so the expected results are the host mirrors' (splat_cases.mirror, rasterize_cases.mirror);
this file holds the point sets and asserts, from the numpy restatements alone (splat_cases.cell_taps, rasterize_cases.footprint, seed_cases.seeding), that they carry what
can go wrong in a splat that sums per leaf and sends the rest through a tail kernel:

  (a) tail and leaf   some voxel receives accepted, non-zero terms both from a point whose cell's leaf exists and from a tail point (cell's leaf absent, or the point does
                      not sort): the one-rounding rule depends on the leaf kernel picking up what the tail kernel left in the accumulator
  (b) empty leaf      some leaf that owns no point receives terms from its neighbours' points: a workgroup whose own range is empty still has work
  (c) crossings       trilinear: terms cross into the +x, the +y, the +z and the +x+y+z neighbour leaf; radial at r = 4: terms arrive from the -1 and the +1 neighbour along
                      every axis and from a corner neighbour
  (d) status classes  those of splat_cases.check_conditions / rasterize_cases.check_conditions

`case(name, kind)` is the stock case of the grid (kind "trilinear": splat_cases.case, "radial": rasterize_cases.case) with TWO PLANTED POINTS in front of it, which supply
(a) on every grid: A a quarter voxel inside the first leaf whose -x neighbour is absent, B a quarter voxel outside it across that face -- B's cell lies in the absent leaf,
so B is a tail point, and both reach the leaf's corner voxel under the cell and under every radius of rasterize_cases.RADII. The stock points supply (c) and (d) as they
are. (b): the stock sets put points into every leaf of the small grids, so (b) is asserted for the prefix of N_EMPTY points, one of the counts the GPU test runs.
one_leaf has no neighbour leaf: (b) and (c) cannot hold there and are asserted for the other grids."""
from __future__ import annotations

import functools

import numpy as np

import points_cases as pc
import rasterize_cases as rc
import seed_cases as sd
import splat_cases as sp

F = np.float32
GRIDS = sp.GRIDS
KINDS = ("trilinear", "radial")
N_PLANTED = 2
N_EMPTY = 65  # (b) is asserted on the first N_EMPTY points: a count of splat_cases.COUNTS
COUNTS = sp.COUNTS + ("all",)  # prefixes of the case's points, and the whole set the conditions are asserted for
assert N_EMPTY in COUNTS
ROWS = ("original", "ranked")


def planted(origins):
    """(A, B): a point of the first leaf whose -x neighbour is absent, and a tail point across that face; both reach the leaf's corner voxel"""
    o = next(np.asarray(q, dtype=np.float64) for q, axis, sign in pc.absent_faces(np.asarray(origins)) if axis == 0 and sign == -1)
    return np.stack([o + [0.25, 0.0, 0.0], o + [-0.25, 0.0, 0.0]]).astype(F)


@functools.lru_cache(maxsize=None)
def case(name, kind="trilinear"):
    """dict(o, vel, phi, xyz, vals, vvals, masks, radii): the stock case behind the planted points; computed once, never written. radii: one per point (radial) or None"""
    stock = sp.case(name) if kind == "trilinear" else rc.case(name)
    o, vel, phi, xyz, vals, vvals, masks = stock[:7]
    front = lambda a, rows: np.ascontiguousarray(np.concatenate([np.asarray(rows, dtype=F), a]))
    c = dict(o=o, vel=vel, phi=phi, masks=masks, xyz=front(xyz, planted(o)), vals=[front(v, [1.5, -2.25]) for v in vals],
             vvals=front(vvals, [[1.5, -0.5, 3.0], [0.75, 2.0, -1.0]]), radii=front(stock[7], [1.0, 1.5]) if kind == "radial" else None)
    for a in [c["xyz"], c["vvals"], *c["vals"]] + ([c["radii"]] if kind == "radial" else []):
        a.setflags(write=False)
    return c


def channel_sets(name, kind="trilinear"):
    """splat_cases.channel_sets over this file's values: {set name: (fields, point values)}"""
    c = case(name, kind)
    phi, vals, vel, vvals = c["phi"], c["vals"], c["vel"], c["vvals"]
    return {"float": ([phi[0]], [vals[0]]), "vec3": ([vel], [vvals]), "float+vec3": ([phi[1], vel], [vals[1], vvals]), "5float+vec3": (phi[:5] + [vel], vals[:5] + [vvals])}


def binned(G, xyz):
    """-> (is each point binned -- it sorts and its cell's leaf exists --, the leaf of its cell or -1): a point that is not binned is a tail point"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    vox = sp.voxel_of(G, pc.cell_of(xyz).astype(np.int64)) if len(xyz) else np.zeros(0, np.int64)
    ok = sd.seeding(xyz) & (vox >= 0)
    return ok, np.where(ok, vox >> 9, -1)


def findings(G, origins, xyz, values, kernel, radius=None):
    """What the restatement says about a point set -> dict(both: voxels with accepted non-zero terms from binned AND tail points, empty_fed: leaves that own no point and
    receive such terms from binned points, steps: the set of (dx, dy, dz) leaf steps from a binned point's leaf to the leaf one of its terms lands in)"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    P, idx, w, _ = rc.taps(G, xyz, kernel, radius, None)
    ok, leaf = binned(G, xyz)
    with np.errstate(all="ignore"):
        x = (w * np.asarray(values, dtype=F)[P]).astype(np.float64) * 2.0 ** 32
        term = (idx >= 0) & (np.abs(x) < 2.0 ** 62)
        term[term] &= np.rint(x[term]) != 0
    from_leaf, from_tail = term & ok[P], term & ~ok[P]
    both = np.intersect1d(idx[from_leaf], idx[from_tail])
    owners = np.bincount(leaf[ok], minlength=len(origins))
    fed = np.unique(idx[from_leaf] >> 9)
    o = np.asarray(origins, dtype=np.int64)
    steps = np.unique((o[idx[from_leaf] >> 9] - o[leaf[P[from_leaf]]]) // 8, axis=0)
    return dict(both=both, empty_fed=fed[owners[fed] == 0], steps=set(map(tuple, steps.tolist())))


TRILINEAR_STEPS = {(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)}
RADIAL_STEPS = {(s if a == 0 else 0, s if a == 1 else 0, s if a == 2 else 0) for a in range(3) for s in (-1, 1)}


def check_conditions(name):
    """(a) .. (d) for the grid's two cases, from the restatement alone"""
    G = sp.oracle_grid(name)  # (asserts (d), trilinear, for the stock points: the planted ones add to classes, they empty none)
    rc.oracle_grid(name)  # ((d), radial)
    several = len(case(name)["o"]) > 1
    for kind, kernel, radii in (("trilinear", "trilinear", (None,)), ("radial", "radial", rc.RADII)):
        c = case(name, kind)
        for radius in radii:
            what = f"{name} {kernel} r={radius}"
            full = findings(G, c["o"], c["xyz"], c["vals"][0], kernel, radius)
            assert len(full["both"]), f"{what}: (a) no voxel receives terms from a binned point and from a tail point"
            head = findings(G, c["o"], c["xyz"][:N_PLANTED], c["vals"][0][:N_PLANTED], kernel, radius)
            assert len(head["both"]), f"{what}: (a) the planted points do not share a voxel"
            if not several:
                continue
            if kernel == "trilinear" or radius == 4.0:  # (the radial kernel: at the radius that reaches furthest)
                few = findings(G, c["o"], c["xyz"][:N_EMPTY], c["vals"][0][:N_EMPTY], kernel, radius)
                assert len(few["empty_fed"]), f"{what}: (b) no leaf without points of its own receives terms at n = {N_EMPTY}"
            if kernel == "trilinear":
                assert TRILINEAR_STEPS <= full["steps"], f"{what}: (c) leaf steps {sorted(full['steps'])}"
            elif radius == 4.0:
                corners = [s for s in full["steps"] if all(abs(d) == 1 for d in s)]
                assert RADIAL_STEPS <= full["steps"] and corners, f"{what}: (c) leaf steps {sorted(full['steps'])}"
