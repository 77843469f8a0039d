"""TEST HELPER of the multigrid tests (tests/test_multigrid.py, tests/test_multigrid_gpu.py, tests/test_multigrid_pool_gpu.py): a numpy mirror of the V-cycle pressure
solve that include/hns.h defines bit for bit ("A second solve method"), written from the header's text, one float32 operation per line. Its fine smoother is the oracle's
red-black sweep (oracle_lib.OracleGrid.rbgs), its residual diag_cases.residual_numpy; the coarse sweep, the transfers and the hierarchy are restated here. A second,
brute-force derivation of the hierarchy -- per voxel on global coordinates, no leaf arithmetic -- is what the mirror's own derivation is held against."""
import numpy as np

import special_cases as sc
from diag_cases import residual_numpy
from hnanosolver_amd import _lib, api, fields
from oracle_lib import OracleGrid

F = np.float32
INV6 = F(0.166666667)
DX = 1.0 / 64.0
Q75, Q25 = F(0.75), F(0.25)


# ---------------------------------------------------------------------------------------------------------------
# leaf sets
# ---------------------------------------------------------------------------------------------------------------


def ordered(o):
    o = np.asarray(o, dtype=np.int32).reshape(-1, 3)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


def ragged_ball(radius=4, drop=0.1, seed=11, shift=(0, 0, 0)):
    """the leaves of a lattice ball with a share of them knocked out: the shape on which a cycle with plain coarse leaf grids diverges"""
    rng = np.random.default_rng(seed)
    r = np.arange(-radius - 1, radius + 2)
    lat = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[((lat + 0.5) ** 2).sum(1) <= radius * radius]
    lat = lat[rng.random(len(lat)) >= drop]
    return ordered(lat * 8 + np.asarray(shift))


def ragged_deep():
    """a ragged set with four levels whose masks above level 1 are not whole octants: a tenth of a 12^3-leaf lattice that starts at a negative, odd leaf coordinate, so a
    level-1 leaf holds anything from one to eight children (whole 4^3 octants), a level-2 leaf 2^3-voxel pieces of them and a level-3 leaf single voxels"""
    rng = np.random.default_rng(23)
    r = np.arange(-5, 7)
    lat = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[rng.random(len(lat)) < 0.11]
    return ordered(lat * 8)


def big_ragged():
    """more than 600 leaves (the 16^3-block fine kernel runs by its own choice), ragged"""
    return ragged_ball(radius=6, drop=0.12, seed=3, shift=(-8, 16, 0))


LEAF_SETS = dict(sc.LEAF_SETS)
LEAF_SETS["ragged_deep"] = ragged_deep


def divergence_for(origins, seed=1):
    """the equality tests' right-hand side: a smooth bump plus noise, so that every level and every bit has something to do"""
    rng = np.random.default_rng(seed)
    c = fields.leaves_to_coords(np.asarray(origins, dtype=np.int32)).astype(np.float64)
    mid, ext = c.mean(0), max(float(np.ptp(c, axis=0).max()), 1.0)
    r2 = (((c - mid) / ext) ** 2).sum(1)
    return (np.exp(-8.0 * r2) * 40.0 + rng.standard_normal(len(c)) * 3.0).astype(F)


def flagship_divergence(origins, R):
    """the convergence tests' right-hand side: what the flagship workload's solve sees -- the divergence of bench.py's synthetic velocity (fields.synthetic_fields at
    extent R) after its self-advection, voxel size 1 / R -> (div, voxel size)"""
    vs = 1.0 / R
    G = OracleGrid(origins)
    adv = G.advect_vector(fields.synthetic_fields(origins, R)["vel"], 1.0 / 24.0, 1.0 / vs)
    return G.divergence(adv, 1.0 / vs), vs


# ---------------------------------------------------------------------------------------------------------------
# the hierarchy
# ---------------------------------------------------------------------------------------------------------------


class Level:
    def __init__(self, origins, mask):
        self.origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
        self.n = len(self.origins)
        self.mask = mask  # (n, 8, 8, 8) bool: the unknowns
        self.nb = api.create_grid_from_leaves(self.origins, 1.0, _lib.HNS_GRID_HOST_ONLY).neighbor_table()
        self.parent = self.octant = self.child = None  # parent / octant: of THIS level's leaves in the level above; child: of this level's leaves in the level below


def coarse_leaves(origins):
    """the distinct floor(origin / 16) * 8, and per fine leaf its parent's index and its octant ox*4 + oy*2 + oz"""
    o = np.asarray(origins, dtype=np.int64)
    co = np.floor_divide(o, 16) * 8
    uniq, parent = np.unique(co, axis=0, return_inverse=True)
    octant = ((o[:, 0] >> 3) & 1) * 4 + ((o[:, 1] >> 3) & 1) * 2 + ((o[:, 2] >> 3) & 1)
    return uniq.astype(np.int32), parent.reshape(-1).astype(np.int64), octant.astype(np.int64)


def build_hierarchy(origins, max_levels=0, exact_masks=True):
    """levels[0] is the given grid (every voxel an unknown). Levels end at one leaf, at max_levels, or where the next level would have no fewer leaves."""
    origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
    levels = [Level(origins, np.ones((len(origins), 8, 8, 8), dtype=bool))]
    while levels[-1].n > 1 and (max_levels == 0 or len(levels) < max_levels):
        fine = levels[-1]
        co, parent, octant = coarse_leaves(fine.origins)
        if len(co) >= fine.n:
            break
        mask = np.zeros((len(co), 8, 8, 8), dtype=bool)
        any_child = fine.mask.reshape(fine.n, 4, 2, 4, 2, 4, 2).any(axis=(2, 4, 6))  # (n, 4, 4, 4): a bit is set iff one of the eight children is an unknown
        child = np.full((len(co), 8), -1, dtype=np.int64)
        for i in range(fine.n):
            ox, oy, oz = (octant[i] >> 2) & 1, (octant[i] >> 1) & 1, octant[i] & 1
            mask[parent[i], 4 * ox:4 * ox + 4, 4 * oy:4 * oy + 4, 4 * oz:4 * oz + 4] = any_child[i]
            child[parent[i], octant[i]] = i
        if not exact_masks:
            mask[:] = True  # the assumed setup that diverges: every voxel of a coarse leaf an unknown
        fine.parent, fine.octant = parent, octant
        levels.append(Level(co, mask))
        levels[-1].child = child
    return levels


def brute_force_level(origins, mask):
    """the next level from the unknowns as global voxel coordinates alone: coarse voxel = floor(i / 2), coarse leaf = floor(I / 8) * 8 -> (origins sorted, {origin: mask})"""
    o = np.asarray(origins, dtype=np.int64)
    out = {}
    for l in range(len(o)):
        loc = np.argwhere(mask[l])
        for I in np.unique(np.floor_divide(o[l] + loc, 2), axis=0):
            leaf = tuple(int(v) for v in np.floor_divide(I, 8) * 8)
            m = out.setdefault(leaf, np.zeros((8, 8, 8), dtype=bool))
            m[tuple(I - np.asarray(leaf))] = True
    return out


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic
# ---------------------------------------------------------------------------------------------------------------


def _shifted(P, nb, axis, d):
    """the field one voxel along `axis` in direction d, 0 where the neighbour leaf is absent (as diag_cases.residual_numpy)"""
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


_PARITY = (np.add.outer(np.add.outer(np.arange(8), np.arange(8)), np.arange(8)) & 1)[None]  # colour 0 (red) = even


def masked_sweeps(L, rhs, p, dx, omega, iterations):
    """`iterations` red-black iterations on a coarse level, on unknowns only (Kernel.cu:621-622 in float32, the sum left to right)"""
    P = np.array(p, dtype=F).reshape(L.n, 8, 8, 8)
    R = np.asarray(rhs, dtype=F).reshape(L.n, 8, 8, 8)
    dx2 = F(dx) * F(dx)
    omega = F(omega)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            for color in (0, 1):
                s = _shifted(P, L.nb, 0, 1) + _shifted(P, L.nb, 0, -1)
                s = s + _shifted(P, L.nb, 1, 1)
                s = s + _shifted(P, L.nb, 1, -1)
                s = s + _shifted(P, L.nb, 2, 1)
                s = s + _shifted(P, L.nb, 2, -1)
                t = R * dx2
                gs = (s - t) * INV6
                d = gs - P
                new = P + omega * d
                P = np.where((_PARITY == color) & L.mask, new, P)
    assert P.dtype == F
    return P.reshape(-1)


def restrict(fine, coarse, rhs_f, p_f, dx):
    """rhs of the coarse level from the fine level's residual; dx: the FINE level's"""
    dx2 = F(dx) * F(dx)
    k = F(-0.75) / dx2
    c = residual_numpy(fine.origins, rhs_f, p_f, F(dx)).reshape(fine.n, 8, 8, 8)
    c = np.where(fine.mask, c, F(0.0))  # +0 at a voxel that is not an unknown
    c = c.reshape(fine.n, 4, 2, 4, 2, 4, 2)
    ch = lambda a, b, d: c[:, :, a, :, b, :, d]  # children indexed dx dy dz
    with np.errstate(all="ignore"):
        s = ((ch(0, 0, 0) + ch(0, 0, 1)) + (ch(0, 1, 0) + ch(0, 1, 1))) + ((ch(1, 0, 0) + ch(1, 0, 1)) + (ch(1, 1, 0) + ch(1, 1, 1)))
        out = np.zeros((coarse.n, 8, 8, 8), dtype=F) * k  # an absent child leaf reads +0: (+0) * k
        for i in range(fine.n):
            o = fine.octant[i]
            ox, oy, oz = (o >> 2) & 1, (o >> 1) & 1, o & 1
            out[fine.parent[i], 4 * ox:4 * ox + 4, 4 * oy:4 * oy + 4, 4 * oz:4 * oz + 4] = s[i] * k
    assert out.dtype == F
    return out.reshape(-1)


def prolong_add(fine, coarse, e, p_f):
    """p_f + the cell-centred trilinear interpolation of the coarse e, on the fine level's unknowns"""
    E = np.asarray(e, dtype=F).reshape(coarse.n, 8, 8, 8)
    pad = np.zeros((coarse.n, 10, 10, 10), dtype=F)  # every coarse leaf with a one-voxel rim out of its 26 neighbours, 0 where absent (a masked voxel holds 0)
    rng = {-1: (slice(0, 1), slice(7, 8)), 0: (slice(1, 9), slice(0, 8)), 1: (slice(9, 10), slice(0, 1))}
    for ax in (-1, 0, 1):
        for ay in (-1, 0, 1):
            for az in (-1, 0, 1):
                leaf = coarse.nb[:, (ax + 1) * 9 + (ay + 1) * 3 + az + 1]
                src = E[np.where(leaf >= 0, leaf, 0)][:, rng[ax][1], rng[ay][1], rng[az][1]].copy()
                src[leaf < 0] = F(0.0)
                pad[:, rng[ax][0], rng[ay][0], rng[az][0]] = src
    ox, oy, oz = (fine.octant >> 2) & 1, (fine.octant >> 1) & 1, fine.octant & 1
    box = np.stack([pad[fine.parent[i], 4 * ox[i]:4 * ox[i] + 6, 4 * oy[i]:4 * oy[i] + 6, 4 * oz[i]:4 * oz[i] + 6] for i in range(fine.n)])  # (n, 6, 6, 6)
    i8 = np.arange(8)
    main = (i8 >> 1) + 1                      # the coarse voxel I = i >> 1, in box coordinates
    other = main + np.where(i8 & 1, 1, -1)    # I + ((i & 1) ? 1 : -1)
    with np.errstate(all="ignore"):
        vz = Q75 * box[:, :, :, main] + Q25 * box[:, :, :, other]  # z first
        vy = Q75 * vz[:, :, main, :] + Q25 * vz[:, :, other, :]    # then y
        v = Q75 * vy[:, main, :, :] + Q25 * vy[:, other, :, :]     # then x
        P = np.asarray(p_f, dtype=F).reshape(fine.n, 8, 8, 8)
        out = np.where(fine.mask, P + v, P)
    assert out.dtype == F
    return out.reshape(-1)


class Mirror:
    """the V-cycle solve on one leaf set"""

    def __init__(self, origins, pre=2, post=2, coarse_iterations=8, max_levels=0, omega=1.0, exact_masks=True):
        self.levels = build_hierarchy(origins, max_levels, exact_masks)
        self.pre, self.post, self.coarse, self.omega = pre, post, coarse_iterations, F(omega)
        self.oracle = OracleGrid(self.levels[0].origins)

    def leaves_per_level(self):
        return [L.n for L in self.levels]

    def sweeps(self, l, rhs, p, dx, iterations):
        if l == 0:
            return self.oracle.rbgs_iterations(rhs, float(dx), float(self.omega), iterations, p0=p)
        return masked_sweeps(self.levels[l], rhs, p, dx, self.omega, iterations)

    def cycle(self, l, rhs, p, dx):
        dx = F(dx)
        if l == len(self.levels) - 1:
            return self.sweeps(l, rhs, p, dx, self.coarse)
        fine, coarse = self.levels[l], self.levels[l + 1]
        p = self.sweeps(l, rhs, p, dx, self.pre)
        rhs_c = restrict(fine, coarse, rhs, p, dx)
        e = self.cycle(l + 1, rhs_c, np.zeros(coarse.n * 512, dtype=F), F(2.0) * dx)
        p = prolong_add(fine, coarse, e, p)
        return self.sweeps(l, rhs, p, dx, self.post)

    def solve(self, div, dx, cycles, each=False):
        """p after `cycles` cycles from p = 0; each: the list of p after every cycle"""
        div = np.ascontiguousarray(div, dtype=F)
        p, out = np.zeros_like(div), []
        for _ in range(cycles):
            p = self.cycle(0, div, p, dx)
            out.append(p)
        return out if each else p

    def history(self, div, dx, cycles):
        """max|c| at p = 0 and after each cycle"""
        o = self.levels[0].origins
        with np.errstate(all="ignore"):
            return [float(np.abs(residual_numpy(o, div, p, F(dx))).max()) for p in [np.zeros_like(div)] + self.solve(div, dx, cycles, each=True)]


def converges(h):
    """the condition of the issue: strictly falling in every cycle, and after the sixth below 1e-2 of the value at p = 0"""
    return all(np.isfinite(h)) and all(b < a for a, b in zip(h[:-1], h[1:])) and h[6] < 1e-2 * h[0]


# ---------------------------------------------------------------------------------------------------------------
# the substep around the solve, through the oracle's kernels (the chain of tests/test_fullsize_gpu.py and tests/dist_reference.py, with the solve handed in)
# ---------------------------------------------------------------------------------------------------------------


def substep_chain(origins, state, names, dt, vs, solve, params=None):
    """hns_sim_core_substep (params None) or hns_sim_substep without a collider on `state` = {"vel", name: array}; solve(div) -> p. -> (state after, p, div)"""
    G = OracleGrid(origins)
    inv_dx = float(F(1.0) / F(vs))
    st = {k: np.array(v, dtype=F) for k, v in state.items()}
    adv = G.advect_vector(st["vel"], dt, inv_dx)
    if params is not None and int(params.factorScale) != 0:
        adv = G.vorticity_confinement(adv, dt, inv_dx, params.vorticityScale, params.factorScale)
    div = G.divergence(adv, inv_dx)
    if params is not None:
        fu, wa, te, fl, div = G.combustion_oxygen(st["fuel"], st["waste"], st["temperature"], div, st["flame"], params.temperatureRelease, params.expansionRate)
        adv = G.temperature_buoyancy(adv, te, dt, params.ambientTemp, params.buoyancyStrength)
        st["fuel"], st["waste"], st["temperature"], st["flame"] = fu, wa, te, fl
    p = solve(div)
    st["vel"] = G.subtract_pressure_gradient(adv, p, inv_dx)
    adv_names = [n for n in names if n != "collision_sdf"]
    for n, out in zip(adv_names, G.advect_scalars(st["vel"], [st[n] for n in adv_names], dt, inv_dx)):
        st[n] = out
    return st, p, div
