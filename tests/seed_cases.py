"""TEST HELPER of tests/test_seed.py (CPU) and tests/test_seed_gpu.py: the seeds of a point set restated in numpy from the text of include/hns.h (never from the C++), the
point sets the seed kernels (hns_seed.hip) are run on, and the host chain a seeded regrid must match byte for byte.

The seeds of a point set: a point seeds iff every coordinate c has -8388608.0f <= c < 8388607.0f (NaN and +-inf fail); its cell is Floor; all eight taps
(i+di, j+dj, k+dk) are seeds whatever their weights; S is the set of leaves (origin = coordinate & ~7) holding a tap, each with a 64-byte mask (byte x*8+y, bit z) of exactly
the tap bits, in OpenVDB leaf order."""
from __future__ import annotations

import functools

import numpy as np

import frame_cases as fc
import points_cases as pc
from hnanosolver_amd import leafio

F = np.float32
N_BALL = 4099
LO, HI = F(-8388608.0), F(8388607.0)


def seeding(xyz):
    x = np.asarray(xyz, dtype=F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return ((x >= LO) & (x < HI)).all(1)


def taps_of(xyz):
    """(m, 8, 3) int64 tap coordinates of the seeding points"""
    x = np.asarray(xyz, dtype=F).reshape(-1, 3)
    cell = np.floor(x[seeding(x)].astype(np.float64)).astype(np.int64)
    corners = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], dtype=np.int64)
    return cell[:, None, :] + corners[None]


def leaf_order(origins):
    """OpenVDB's leaf order: signed root tile (coordinate >> 12) x, y, z; then the child offset in the 4096^3 node; then in the 128^3 node"""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 3)
    upper = ((o[:, 0] & 4095) >> 7) << 10 | ((o[:, 1] & 4095) >> 7) << 5 | ((o[:, 2] & 4095) >> 7)
    lower = ((o[:, 0] & 127) >> 3) << 8 | ((o[:, 1] & 127) >> 3) << 4 | ((o[:, 2] & 127) >> 3)
    return np.lexsort((lower, upper, o[:, 2] >> 12, o[:, 1] >> 12, o[:, 0] >> 12))


def seeds(xyz):
    """-> (origins (m, 3) int32 in OpenVDB leaf order, masks (m, 64) uint8, the number of points that do not seed)"""
    x = np.asarray(xyz, dtype=F).reshape(-1, 3)
    skipped = int((~seeding(x)).sum())
    t = taps_of(x).reshape(-1, 3)
    if len(t) == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 64), np.uint8), skipped
    leaves, inv = np.unique(t & ~7, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = leaf_order(leaves)
    rank = np.empty(len(leaves), dtype=np.int64)
    rank[order] = np.arange(len(leaves))
    local = t & 7
    masks = np.zeros((len(leaves), 64), dtype=np.uint8)
    np.bitwise_or.at(masks, (rank[inv], local[:, 0] * 8 + local[:, 1]), (1 << local[:, 2]).astype(np.uint8))
    return leaves[order].astype(np.int32), masks, skipped


def same(a, b):
    """two (origins, masks, skipped) triples, as bytes"""
    return (np.asarray(a[0]).shape == np.asarray(b[0]).shape and np.asarray(a[0], np.int32).tobytes() == np.asarray(b[0], np.int32).tobytes()
            and np.asarray(a[1], np.uint8).tobytes() == np.asarray(b[1], np.uint8).tobytes() and int(a[2]) == int(b[2]))


# ---- point sets ----------------------------------------------------------------------------------------------------------------------------------------------------------


def emitter_ball(corner, seed=0, n=N_BALL, radius=3.0):
    """n points within `radius` voxels of a leaf corner: eight leaves under one wave's points, most lanes of a wave on the same key"""
    rng = np.random.default_rng([seed, 77])
    d = rng.standard_normal((n, 3))
    d *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return np.ascontiguousarray((np.asarray(corner, dtype=np.float64) + d).astype(F))


def outside_corner(origins):
    """a leaf corner outside the domain, one leaf beyond its +x end: none of the eight leaves around it is a leaf of the domain"""
    o = np.asarray(origins, dtype=np.int64)
    top = o[np.argmax(o[:, 0])]
    corner = top + np.array([24, 8, 8])
    have = set(map(tuple, o.tolist()))
    for d in range(8):
        assert tuple((corner - 8 + 8 * np.array([d >> 2, (d >> 1) & 1, d & 1])).tolist()) not in have
    return corner


def repeats(n=N_BALL):
    return np.ascontiguousarray(np.tile(np.array([[13.25, -2.5, 7.75]], dtype=F), (n, 1)))


def edges():
    """the ends of the seeding range, the values that never seed, -0.0f and exact integers, each on every axis beside coordinates that seed, and together"""
    below = np.nextafter(LO, F(-np.inf))
    special = [LO, below, F(8388606.5), HI, F(np.inf), F(-np.inf), F(np.nan), F(-0.0), F(0.0), F(7.0), F(8.0), F(-8.0), F(-1.0), F(8388606.0), F(-8388607.5)]
    rows = []
    for v in special:
        for axis in range(3):
            p = np.array([3.25, -5.5, 70.0], dtype=F)
            p[axis] = v
            rows.append(p)
        rows.append(np.array([v, v, v], dtype=F))
    rows.append(np.array([LO, F(8388606.5), F(-0.0)], dtype=F))
    return np.ascontiguousarray(np.stack(rows))


SPECIAL_SETS = {
    "ball": lambda: emitter_ball((64, -8, 16)),
    "repeats": repeats,
    "edges": edges,
}


@functools.lru_cache(maxsize=None)
def point_set(name, count=None):
    """a named point set, computed once and never written: a grid of points_cases.GRIDS (its first `count` points) or one of SPECIAL_SETS"""
    xyz = SPECIAL_SETS[name]() if name in SPECIAL_SETS else pc.case(name)[3][:count]
    xyz = np.ascontiguousarray(xyz, dtype=F)
    xyz.setflags(write=False)
    return xyz


def all_point_sets():
    return [(g, n) for g in pc.GRIDS for n in pc.COUNTS] + [(k, None) for k in SPECIAL_SETS]


def share_with_a_tap_outside(G, xyz):
    """the share of points with a tap outside the domain, on the ORACLE's count"""
    return float((pc.taps_inside(G, xyz) < 8).mean())


# ---- the host chain of a seeded regrid -------------------------------------------------------------------------------------------------------------------------------------


def host_chain_seeded(origins, masks, state, names, p, xyz, sources=None, sdf=None):
    """What hns_sim_regrid_seeded stands for: domain and masks from frame_cases.host_chain with a zero-valued velocity source over S merged in (leafio.add_leaves), fields
    from the UNSEEDED host_chain gathered onto that domain with the usual fills -> (origins, masks, state)"""
    so, sm, _ = seeds(xyz)
    zero = (so, sm, np.zeros((len(so) * 512, 3), dtype=F))
    merged = dict(sources or {})
    vel_key = next((k for k, v in merged.items() if fc.is_velocity(v[2])), None)
    if vel_key is None:
        merged["vel"] = zero
    else:
        o2, m2, _ = leafio.add_leaves(merged[vel_key], zero, 3)
        merged[vel_key] = (o2, m2, np.zeros((len(o2) * 512, 3), dtype=F))  # (only its leaves and masks are used)
    dom, dm, _ = fc.host_chain(origins, masks, state, names, p, merged, sdf)
    dom0, _, out0 = fc.host_chain(origins, masks, state, names, p, sources, sdf)
    assert set(map(tuple, dom0.tolist())) <= set(map(tuple, dom.tolist())), "the unseeded domain is a subset of the seeded one"
    out = {"vel": leafio.gather_leaves(dom, dom0, out0["vel"], 3, leafio.FILL_ZERO)}
    for n in names:
        out[n] = leafio.gather_leaves(dom, dom0, out0[n], 1, leafio.FILL_SDF if n == "collision_sdf" else leafio.FILL_ZERO)
    return dom, dm, out
