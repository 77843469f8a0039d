"""TEST HELPER of tests/test_points_cases.py (CPU) and tests/test_points_gpu.py: the point sets the point kernels (hns_points.hip) are sampled and traced at, the conditions
those sets must meet -- counted by the ORACLE, never by the kernel under test --, and the mirror of k_trace_points: numpy float32, one rounded operation per line, with
U(x) the oracle's sample_trilinear_v on the fmaf branch of the Vec3f lerp (Stencils.hpp:131-135), which the advection kernels are pinned to.

Point classes, generated per grid from its leaf origins (shares of the 4,099-point set):
  inside     34 %  cells wholly inside one leaf
  crossing   12 %  the lower corner on local index 7 along one, two and three axes: 2, 4, 8 leaves under the cell
  rim        20 %  cells astride a face whose neighbour leaf is absent: half their taps outside
  outside    12 %  cells wholly inside an absent leaf that touches the domain
  far         5 %  thousands of voxels away
  integer     6 %  exact integer positions
  below       6 %  one to three ulps below an integer, negative integers and -0's neighbour included
  large       5 %  magnitudes from 2^16 to 2^22, both signs
"""
from __future__ import annotations

import functools

import numpy as np

import special_cases as sc
from oracle_lib import OracleGrid, oracle, oracle_device

F = np.float32
N_POINTS = 4099
COUNTS = (0, 1, 63, 64, 65, 257, 4099)  # the tails of a wave and of a 256-thread workgroup
GRIDS = ("one_leaf", "ragged32", "ragged32_off_origin", "sparse_far", "dense32")
DT, INV_DX = 0.04, 24.0  # s = dt * inv_dx is no power of two: its products round
SPEEDS = (0.5, 4.0, 30.0)  # voxels per step: the same leaf, a neighbour leaf, beyond the neighbour tables


def absent_faces(origins):
    """(leaf origin, axis, sign) of every leaf face whose neighbour leaf is absent"""
    have = set(map(tuple, origins.tolist()))
    out = []
    for o in origins.tolist():
        for axis in range(3):
            for sign in (-1, 1):
                q = list(o)
                q[axis] += 8 * sign
                if tuple(q) not in have:
                    out.append((o, axis, sign))
    return out


def make_points(origins, seed, n=N_POINTS):
    rng = np.random.default_rng([seed, 41])
    origins = np.asarray(origins, dtype=np.int64)
    share = {"inside": 0.34, "crossing": 0.12, "rim": 0.20, "outside": 0.12, "far": 0.05, "integer": 0.06, "below": 0.06}
    k = {c: int(round(s * n)) for c, s in share.items()}
    k["large"] = n - sum(k.values())

    def leaves(m):
        return origins[rng.integers(0, len(origins), m)].astype(np.float64)

    parts = [leaves(k["inside"]) + rng.uniform(0.0, 6.99, (k["inside"], 3))]
    p = leaves(k["crossing"]) + rng.uniform(0.0, 6.99, (k["crossing"], 3))
    for row in range(k["crossing"]):
        axes = rng.permutation(3)[: 1 + row % 3]
        p[row, axes] = np.floor(p[row, axes] / 8.0) * 8.0 + 7.0 + rng.uniform(0.01, 0.99, len(axes))
    parts.append(p)
    faces = absent_faces(origins)
    for cls in ("rim", "outside"):
        p = np.empty((k[cls], 3))
        for row in range(k[cls]):
            o, axis, sign = faces[rng.integers(0, len(faces))]
            p[row] = np.asarray(o, dtype=np.float64) + rng.uniform(0.0, 6.99, 3)
            if cls == "rim":  # the cell whose two layers along `axis` lie either side of the face
                p[row, axis] = o[axis] - rng.uniform(0.01, 0.99) if sign < 0 else o[axis] + 7.0 + rng.uniform(0.01, 0.99)
            else:  # inside the absent leaf, away from its faces
                p[row, axis] = o[axis] + 8.0 * sign + rng.uniform(0.0, 6.99)
        parts.append(p)
    parts.append(leaves(k["far"]) + rng.choice([-1.0, 1.0], (k["far"], 3)) * rng.uniform(2000.0, 9000.0, (k["far"], 3)))
    parts.append(leaves(k["integer"]) + rng.integers(-2, 11, (k["integer"], 3)))
    b = (leaves(k["below"]) + rng.integers(-1, 10, (k["below"], 3))).astype(F)
    b[:5, 0] = np.array([0.0, -1.0, -8.0, 8.0, -16.0], dtype=F)[: len(b[:5])]
    for _ in range(3):
        step = rng.random(b.shape) < 0.6
        b = np.where(step, np.nextafter(b, F(-np.inf)), b)
    b = np.where(b == np.floor(b), np.nextafter(b, F(-np.inf)), b)  # (every one at least one ulp below)
    parts.append(b.astype(np.float64))
    parts.append(rng.choice([-1.0, 1.0], (k["large"], 3)) * np.exp2(rng.uniform(16.0, 22.0, (k["large"], 3))))
    xyz = np.concatenate(parts).astype(F)
    assert xyz.shape == (n, 3)
    return np.ascontiguousarray(xyz[rng.permutation(n)])


def cell_of(xyz):
    """Floor with the GPU's conversion: saturating, NaN -> 0 (int32)"""
    with np.errstate(invalid="ignore"):
        f = np.floor(np.where(np.isnan(xyz), F(0), xyz).astype(np.float64))
    return np.clip(f, -(2.0 ** 31), 2.0 ** 31 - 1).astype(np.int32)


def taps_inside(G: OracleGrid, xyz):
    """how many of the eight taps of each position's cell the ORACLE finds inside the domain"""
    ones = np.ones(G.N, dtype=F)
    ijk = cell_of(xyz).astype(np.int64)
    count = np.zeros(len(xyz), dtype=np.int64)
    for c in range(8):
        t = ijk + np.array([c >> 2, (c >> 1) & 1, c & 1])
        ok = (np.abs(t) < 2 ** 31 - 16).all(1)
        count += np.where(ok, G.sample_nearest_f(ones, np.where(ok[:, None], t, 0).astype(np.int32)), 0).astype(np.int64)
    return count


def leaf_exists(G: OracleGrid, xyz):
    """is the cell of each position in a leaf of the domain (by the oracle)?"""
    ones = np.ones(G.N, dtype=F)
    return G.sample_nearest_f(ones, cell_of(xyz)) == F(1)


def check_conditions(G: OracleGrid, xyz, name):
    """the shares the issue sets for the 4,099-point set of every grid but one_leaf, on the oracle's count"""
    c = taps_inside(G, xyz)
    full, part, none = float((c == 8).mean()), float(((c > 0) & (c < 8)).mean()), float((c == 0).mean())
    assert full >= 0.30 and part >= 0.10 and none >= 0.05, f"{name}: all eight inside {full:.3f}, one to seven {part:.3f}, none {none:.3f}"
    return full, part, none


@functools.lru_cache(maxsize=None)
def case(name):
    """(origins, velocity of unit scale, eleven float fields, the 4,099 points) of a grid: computed once, never written"""
    o = np.ascontiguousarray(sc.LEAF_SETS[name](), dtype=np.int32)
    rng = np.random.default_rng([23, GRIDS.index(name)])
    N = len(o) * 512
    vel = rng.standard_normal((N, 3)).astype(F)
    phi = [rng.standard_normal(N).astype(F) for _ in range(11)]
    xyz = make_points(o, GRIDS.index(name))
    for a in [vel, xyz, *phi]:
        a.setflags(write=False)
    return o, vel, phi, xyz


def scaled_velocity(vel, speed, s):
    """displacements of about `speed` voxels per step of scaled time step s"""
    return (vel * F(speed / (abs(float(s)) * 1.6))).astype(F)


class fma_branch:
    """the oracle's Vec3f lerp on its device branch for the block; the default (the same branch) is restored afterwards, as tests/test_oracle_pins.py does"""

    def __init__(self, *libs):
        self.libs = libs or (oracle(),)

    def __enter__(self):
        for L in self.libs:
            L.orc_set_vec3_lerp_fma(1)

    def __exit__(self, *exc):
        for L in self.libs:
            L.orc_set_vec3_lerp_fma(1)


def trace_mirror(G: OracleGrid, vel, xyz, dt, inv_dx, order, steps):
    """k_trace_points restated: -> (positions after every step, [steps + 1, n, 3] with the start first; status bytes after the last)"""
    s = F(dt) * F(inv_dx)
    h = F(0.5) * s
    s6 = s * F(0.16666667)
    two = F(2.0)
    x = np.array(xyz, dtype=F)
    path = [x.copy()]
    U = lambda q: G.sample_trilinear_v(vel, q)
    with np.errstate(all="ignore"), fma_branch(G.L):
        for _ in range(steps):
            k1 = U(x)
            if order == 1:
                d = s * k1
                x = x + d
            elif order == 2:
                d = h * k1
                mid = x + d
                k2 = U(mid)
                d = s * k2
                x = x + d
            else:
                d = h * k1
                k2 = U(x + d)
                d = h * k2
                k3 = U(x + d)
                d = s * k3
                k4 = U(x + d)
                t = two * k2
                acc = k1 + t
                t = two * k3
                acc = acc + t
                acc = acc + k4
                d = s6 * acc
                x = x + d
            x = x.astype(F)
            path.append(x.copy())
    status = (np.isfinite(x).all(1) & leaf_exists(G, x)).astype(np.uint8)
    return np.stack(path), status
