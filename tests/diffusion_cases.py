"""TEST HELPER of tests/test_diffusion_*.py: the numpy mirror of "DIFFUSING A SIM" (include/hns.h), restated from the header's text alone, and the fixture the CPU and
the GPU tests share. The mirror is written once over a dtype: in float32 every line is the one rounded operation the header states, and the kernels of hns_diffusion.hip
must equal it in every word; in float64 the same text is the yardstick of the mathematics.

Voxels are rows of flat arrays in leaf order, voxel x << 6 | y << 3 | z of leaf l at row 512 l + that, as the library lays fields out."""
import functools

import numpy as np

from frame_cases import random_leaves, random_masks, unpack

FACES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))  # the header's fixed order: +x, -x, +y, -y, +z, -z
METHODS = {"jacobi": 0, "chebyshev": 1}


def coords(origins):
    """(L * 512, 3) global voxel coordinates in row order"""
    n = np.arange(512)
    local = np.stack([n >> 6, (n >> 3) & 7, n & 7], 1)
    return (np.asarray(origins, np.int64)[:, None, :] + local[None]).reshape(-1, 3)


def neighbours(origins):
    """(6, N) the row of every voxel's face neighbour in the header's order, -1 where its leaf is absent"""
    origins = np.asarray(origins, np.int64)
    leaf_of = {tuple(o): l for l, o in enumerate(origins.tolist())}
    ijk = coords(origins)
    out = np.empty((6, len(ijk)), np.int64)
    for f, d in enumerate(FACES):
        q = ijk + np.array(d)
        org = q & ~7
        leaf = np.array([leaf_of.get(tuple(o), -1) for o in org.tolist()])
        loc = ((q[:, 0] & 7) << 6) | ((q[:, 1] & 7) << 3) | (q[:, 2] & 7)
        out[f] = np.where(leaf < 0, -1, leaf * 512 + loc)
    return out


def classes(n, active=None, sdf=None, collide=False, threshold=0.0):
    """(unknown, solid), (N,) bool each. active: (N,) bool or None = every voxel; sdf: the collision_sdf field, read only with collide. A NaN is not solid."""
    with np.errstate(invalid="ignore"):
        solid = (np.asarray(sdf, np.float32) < np.float32(threshold)) if collide else np.zeros(n, bool)
    unknown = (np.ones(n, bool) if active is None else np.asarray(active, bool).reshape(-1)) & ~solid
    return unknown, solid


def faces(nb, unknown, solid):
    """(open, wall), (6, N) bool each, of the unknowns (all False elsewhere)"""
    there = nb >= 0
    at = np.where(there, nb, 0)
    return there & unknown[at] & unknown[None], there & solid[at] & unknown[None]


def schedule(coefficient, dt, voxel_size, iterations, dtype=np.float32):
    """the host constants, one rounded operation per step: {"a", "r" [7], "rho", "omega" [256]}; omega[k - 1] = w_k up to `iterations`, 0 behind"""
    T = dtype
    with np.errstate(all="ignore"):
        h2 = T(voxel_size) * T(voxel_size)
        a = T(coefficient) * T(dt)
        a = a / h2
        r = np.empty(7, T)
        for m in range(7):
            e = a * T(m)
            den = T(1) + e
            r[m] = T(1) / den
        s = T(6) * a
        den = T(1) + s
        rho = s / den
        q = rho * rho
        omega = np.zeros(max(256, iterations), T)  # (the ABI holds 256; the mirror runs longer for its own limit)
        omega[0] = T(1)
        if iterations >= 2:
            h = q * T(0.5)
            d = T(1) - h
            omega[1] = T(1) / d
        c = q * T(0.25)
        for k in range(2, iterations):
            e = c * omega[k - 1]
            d = T(1) - e
            omega[k] = T(1) / d
    return {"a": a, "r": r, "rho": rho, "omega": omega}


def iterate(b, nb, open_, count, unknown, sch, iterations, method, dtype=np.float32, every=None):
    """x^iterations of one field. b: (N,) or (N, 3) for the velocity; count: (N,) the m of every voxel (open faces; for the velocity open + wall faces). Voxels that
    are no unknowns keep b's bytes. every: a function called with (k, x^k) for every iterate."""
    T = dtype
    b = np.asarray(b, T)
    vec = b.ndim == 2
    a, r, w = T(sch["a"]), np.asarray(sch["r"], T)[count], np.asarray(sch["omega"], T)
    at = np.where(nb >= 0, nb, 0)
    op = open_[:, :, None] if vec else open_
    un = unknown[:, None] if vec else unknown
    if vec:
        r = r[:, None]
    x, before = b, None
    with np.errstate(all="ignore"):
        for k in range(1, iterations + 1):
            S = np.zeros_like(b)
            for f in range(6):
                S = np.where(op[f], S + x[at[f]], S)
            t = a * S
            t = b + t
            j = t * r
            if method == 0 or k == 1:
                new = j
            else:
                d = j - before
                d = w[k - 1] * d
                new = before + d
            new = np.where(un, new, b).astype(T)
            before, x = x, new
            if every is not None:
                every(k, x)
    return x


def apply_mirror(origins, state, dt, voxel_size, fields, viscosity=0.0, iterations=8, method="jacobi", collide=False, threshold=0.0, active=None, dtype=np.float32, nb=None):
    """what hns_diffusion_apply leaves of `state` ({"vel": (N, 3), name: (N,)}): a new dict; only the listed fields with a != 0 (and "vel" with viscosity) are new arrays.
    nb: neighbours(origins), where the caller has them already"""
    n = len(origins) * 512
    nb = neighbours(origins) if nb is None else nb
    unknown, solid = classes(n, active, state.get("collision_sdf"), collide, threshold)
    open_, wall = faces(nb, unknown, solid)
    m_open, m_wall = open_.sum(0), wall.sum(0)
    out = dict(state)
    sch = schedule(viscosity, dt, voxel_size, iterations, dtype)
    if sch["a"] != 0:
        out["vel"] = iterate(state["vel"], nb, open_, m_open + m_wall, unknown, sch, iterations, METHODS[method], dtype)
    for name, coefficient in (fields or {}).items():
        sch = schedule(coefficient, dt, voxel_size, iterations, dtype)
        if sch["a"] != 0:
            out[name] = iterate(state[name], nb, open_, m_open, unknown, sch, iterations, METHODS[method], dtype)
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------

BLOCK = np.array([[x, y, z] for x in (-8, 0) for y in (-8, 0) for z in (-8, 0)], np.int32)  # a 2 x 2 x 2 block of leaves round the origin
BOXES = ((0, 3), (-4, -1))  # two solid boxes [lo, hi]^3: they touch the block's inner leaf planes from either side


@functools.lru_cache(maxsize=None)
def fixture():
    """{"origins": (25, 3) int32, "masks": (25, 64) uint8, "active": (N,) bool, "sdf": (N,) float32 -- solid below 0 --, "nb": (6, N)}. Some twenty random leaves with
    negative origins and a lone leaf, plus the block: the random leaves alone have no z-adjacent pair with an open face between them, and an origin-centred sphere puts
    no wall face across a leaf plane. The conditions the tests rest on are asserted here, so that a later edit cannot thin the coverage silently."""
    origins = np.unique(np.concatenate([random_leaves(7, n=20, span=3), BLOCK]), axis=0).astype(np.int32)
    L = len(origins)
    bits = unpack(random_masks(5, L))
    bits[L // 2:] |= np.random.default_rng(3).random((L - L // 2, 512)) < 0.7
    in_block = (origins[:, None, :] == BLOCK[None]).all(2).any(1)
    assert in_block.sum() == 8
    bits[in_block] = True
    ijk = coords(origins)
    d = [np.maximum(lo - ijk, ijk - hi).max(1) for lo, hi in BOXES]  # Chebyshev box distances: <= 0 inside
    sdf = (np.minimum(d[0], d[1]) - 0.5).astype(np.float32)
    nb = neighbours(origins)
    active = bits.reshape(-1)
    out = {"origins": origins, "masks": np.packbits(bits.reshape(L, 64, 8), axis=2, bitorder="little").reshape(L, 64), "active": active, "sdf": sdf, "nb": nb}
    cross = np.stack([(np.arange(L * 512) // 512) != (np.where(nb[f] >= 0, nb[f], 0) // 512) for f in range(6)])
    for collide in (False, True):
        unknown, solid = classes(L * 512, active, sdf, collide, 0.0)
        open_, wall = faces(nb, unknown, solid)
        assert (open_ & cross).any(1).all(), "a direction without an open face across a leaf boundary"
        assert set(np.unique(open_.sum(0)[unknown])) == set(range(7)), "a face count m that no unknown has"
        assert (~unknown.reshape(L, 512).any(1)).any(), "no leaf without unknowns"
        if collide:
            assert (wall & cross).any(1).all(), "a direction without a wall face across a leaf boundary"
            assert set(np.unique((open_ | wall).sum(0)[unknown])) == set(range(7))
        out["counts", collide] = {"unknowns": int(unknown.sum()), "solid": int(solid.sum()), "open_across": (open_ & cross).sum(1).tolist(),
                                  "wall_across": (wall & cross).sum(1).tolist(), "empty_leaves": int((~unknown.reshape(L, 512).any(1)).sum())}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
