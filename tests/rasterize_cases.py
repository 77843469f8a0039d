"""TEST HELPER of tests/test_rasterize.py (CPU) and tests/test_rasterize_gpu.py: points rasterised into fields under a spec (include/hns.h: hns_splat_spec) -- a radius
footprint in place of the trilinear cell, a weighted average in place of the sum.

`restate` is the header's text written again in numpy, from the header alone: float32 arrays so that every line rounds once, the box and the weights of every candidate
voxel of every point at once, leaf lookup through the ORACLE's grid (splat_cases.voxel_of), the sums by np.add.at on int64. The trilinear kernel's cell and weights are
splat_cases.cell_taps. The host mirror hns_grid_splat_points_spec is held to it in every byte on the CPU; the device is held to the host mirror on the GPU.

`case(name)` is splat_cases.case's fields, points and values with more points mixed in (`extra_points`): integer positions, positions exactly r away from a voxel along
one, two and three axes for every radius of RADII, boxes that straddle eight leaves, coordinate 0 and -0.0, negative coordinates, footprints that hang out of the domain,
positions that do not rasterise (NaN, inf, beyond the seeds' range) and cell centres (an empty footprint at r = 0.4). The conditions are asserted in `check_conditions`,
on the CPU, from the restatement alone.
"""
from __future__ import annotations

import functools

import numpy as np

import splat_cases as sp
from oracle_lib import OracleGrid

F = np.float32
GRIDS = sp.GRIDS
RADII = (0.5, 1.0, 1.5, 2.5, 4.0)
GROUP_RADII = {1: 0.5, 4: 1.0, 16: 1.5, 64: 4.0}  # lanes per point of the device kernel: one radius each
COUNTS = sp.COUNTS + (3, 5, 15, 17)  # and the tails of a group of lanes
SUBNORMAL = np.float32(1e-41)
SPECIAL_RADII = np.array([0.0, -1.0, np.nan, np.inf, SUBNORMAL, 4.0, np.nextafter(F(4.0), F(np.inf)), 0.4], dtype=F)


def extra_points(origins, seed):
    rng = np.random.default_rng([seed, 77])
    o = np.asarray(origins, dtype=np.float64)
    pick = lambda m: o[rng.integers(0, len(o), m)]
    parts = [pick(24) + rng.integers(0, 8, (24, 3))]  # integer positions inside leaves
    for r in RADII:  # exactly r away from the voxel v along one, two, three axes, either side: that voxel's q is 1, 2 or 3 -- outside; its neighbours decide the rounding
        v = pick(6) + rng.integers(0, 8, (6, 3))
        shift = np.array([[r, 0, 0], [0, -r, 0], [r, r, 0], [0, -r, r], [r, r, r], [-r, -r, -r]])
        parts.append(v + shift)
    parts.append(pick(12) + 7.5 + rng.uniform(-0.4, 0.4, (12, 3)))  # round a leaf's upper corner: the box straddles eight leaves from r = 1 on
    parts.append(pick(6) - rng.uniform(0.05, 3.9, (6, 3)))  # below a leaf's lower corner: part of the footprint hangs out where the neighbour is absent
    parts.append(np.array([[0.0, 0.0, 0.0], [-0.0, 0.5, 0.0], [0.0, -0.25, 3.0], [-1.0, -1.0, -1.0], [-7.5, -8.0, -8.5]]))
    parts.append(pick(6) + rng.integers(0, 7, (6, 3)) + 0.5)  # cell centres
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [8388607.0, 1, 1], [1, -8388609.0, 1], [3e9, 3e9, 3e9], [8388606.5, 1, 1], [-8388608.0, 1, 1]])
    return np.concatenate(parts + [bad]).astype(F)


@functools.lru_cache(maxsize=None)
def case(name):
    """(origins, velocity, float fields, points, point values per float field, point values of the velocity, masks, one radius per point): computed once, never written"""
    o, vel, phi, xyz, vals, vvals, masks = sp.case(name)
    rng = np.random.default_rng([83, GRIDS.index(name)])
    extra = extra_points(o, GRIDS.index(name))
    pts = np.concatenate([xyz, extra])
    order = rng.permutation(len(pts))
    more = lambda v: np.concatenate([v, (rng.standard_normal((len(extra), *v.shape[1:])) * 3.0).astype(F)])[order]
    pts, vals, vvals = np.ascontiguousarray(pts[order]), [np.ascontiguousarray(more(v)) for v in vals], np.ascontiguousarray(more(vvals))
    radii = rng.choice(np.array([0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.3, 4.0], dtype=F), len(pts))
    at = rng.permutation(len(pts))[: 4 * len(SPECIAL_RADII)]
    radii[at] = np.tile(SPECIAL_RADII, 4)
    inside = np.flatnonzero(np.isfinite(pts).all(1))[:8]  # and the special radii on points that sit in the domain: the cell centres of the first leaf
    pts = np.array(pts)
    pts[inside] = o[0].astype(F) + F(3.5)
    radii[inside] = SPECIAL_RADII
    for a in [pts, vvals, radii, *vals]:
        a.setflags(write=False)
    return o, vel, phi, pts, vals, vvals, masks, radii


def rasterises(xyz, r, bound):
    with np.errstate(invalid="ignore"):
        return ((xyz >= F(-8388608.0)) & (xyz < F(8388607.0))).all(1) & (r > F(0.0)) & (r <= F(bound))


def box_of(xyz, r, ok):
    """-> (lo [n, 3] int64, E [n] int64; E = 0 for a point that does not rasterise)"""
    with np.errstate(all="ignore"):
        low = xyz - r[:, None]
        twice = F(2.0) * r
        assert low.dtype == F and twice.dtype == F
        lo = np.where(ok[:, None], np.floor(low), 0).astype(np.int64) + 1
        E = np.where(ok, np.ceil(twice), 0).astype(np.int64)
    assert E.max(initial=0) <= 8
    return lo, E


def footprint(G: OracleGrid, xyz, r, bound):
    """the header's radial footprint -> (P point of every footprint voxel, idx its flat voxel or -1, w its weight, ijk), grouped by point"""
    xyz, r = np.asarray(xyz, dtype=F).reshape(-1, 3), np.asarray(r, dtype=F)
    n = len(xyz)
    lo, E = box_of(xyz, r, rasterises(xyz, r, bound))
    count = E ** 3
    P = np.repeat(np.arange(n), count)
    m = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
    e = E[P]
    ijk = lo[P] + np.stack([m // (e * e), (m // e) % e, m % e], 1)
    with np.errstate(all="ignore"):
        d = ijk.astype(F) - xyz[P]
        xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
        s = xx + yy
        d2 = s + zz
        r2 = r * r
        inv = F(1.0) / r2
        q = d2 * inv[P]
        inside = q < F(1.0)
        a = F(1.0) - q
        w = a * a
    assert w.dtype == F
    P, ijk, w = P[inside], ijk[inside], w[inside]
    idx = sp.voxel_of(G, ijk) if len(P) else np.zeros(0, np.int64)
    return P, idx, w, ijk


def taps(G, xyz, kernel, radius, radii):
    """-> (P, idx, w, status) of either kernel: every candidate of every point, landed or not"""
    n = len(xyz)
    if kernel == "trilinear":
        idx, w, _ = sp.cell_taps(G, xyz)
        return np.repeat(np.arange(n), 8), idx.reshape(-1), w.reshape(-1), (idx >= 0).sum(1).astype(np.uint8)
    r = np.full(n, F(radius)) if radii is None else np.asarray(radii, dtype=F)
    P, idx, w, _ = footprint(G, xyz, r, radius)
    nf, nl = np.bincount(P, minlength=n), np.bincount(P[idx >= 0], minlength=n)
    return P, idx, w, np.where((nf > 0) & (nl == nf), 2, np.where(nl > 0, 1, 0)).astype(np.uint8)


def restate(G: OracleGrid, fields, xyz, values, log2_quantum, kernel="trilinear", mode="add", radius=None, radii=None, min_weight=0.0, masks=None, activate=True, cached=None):
    """The header's text in numpy -> (new fields, status, rejected, new masks or None). cached: the result of `taps` for these points (it does not depend on the rest)"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    P, idx, w, status = cached if cached is not None else taps(G, xyz, kernel, radius, radii)
    landed = idx >= 0
    new_masks = None
    if masks is not None:
        new_masks = np.array(masks, dtype=np.uint8).reshape(-1)
        if activate:
            with np.errstate(invalid="ignore"):
                on = landed & (w > 0)
            np.bitwise_or.at(new_masks, idx[on] >> 3, (1 << (idx[on] & 7)).astype(np.uint8))
        new_masks = new_masks.reshape(np.asarray(masks).shape)
    scale, quantum = 2.0 ** (-log2_quantum), 2.0 ** log2_quantum

    def accumulate(v):
        """-> (the int64 accumulators of a channel whose point values are v, its landed terms that were not accepted)"""
        with np.errstate(all="ignore"):
            t = w * v[P]
            assert t.dtype == F
            x = t.astype(np.float64) * scale
            accepted = landed & (np.abs(x) < 2.0 ** 62)
        acc = np.zeros(G.N, dtype=np.int64)
        np.add.at(acc, idx[accepted], np.rint(x[accepted]).astype(np.int64))
        return acc, int((landed & ~accepted).sum())

    total = lambda a: (a.astype(np.float64) * quantum).astype(F)
    if mode == "average":
        a_w, none = accumulate(np.ones(len(xyz), dtype=F))
        assert none == 0  # (a weight's term is always accepted)
        nz_w = np.flatnonzero(a_w)
    out, rejected = [], 0
    for field, vals in zip(fields, values):
        new = np.array(field, dtype=F)
        ncomp = new.size // G.N
        flat, v = new.reshape(G.N, ncomp), np.asarray(vals, dtype=F).reshape(len(xyz), ncomp)
        for comp in range(ncomp):
            a_v, rej = accumulate(np.ascontiguousarray(v[:, comp]))
            rejected += rej
            with np.errstate(all="ignore"):
                if mode == "average":
                    wsum, vsum = total(a_w[nz_w]), total(a_v[nz_w])
                    den = np.maximum(wsum, F(min_weight))
                    flat[nz_w, comp] = vsum / den
                else:
                    nz = np.flatnonzero(a_v)
                    flat[nz, comp] = flat[nz, comp] + total(a_v[nz])
        assert new.dtype == F
        out.append(new)
    return out, status, rejected, new_masks


def check_conditions(G: OracleGrid, xyz, name):
    """what the point set of a grid must hold, counted from the restatement"""
    xyz = np.asarray(xyz, dtype=F)
    finite = np.isfinite(xyz).all(1)
    assert ((xyz == np.floor(xyz)).all(1) & finite).sum() >= 24 and (xyz == 0).any() and (xyz < 0).any() and not finite.all(), name
    for radius in RADII:
        r = np.full(len(xyz), F(radius))
        ok = rasterises(xyz, r, radius)
        assert ok.any() and not ok[finite].all(), f"{name}: points that do not rasterise"
        lo, E = box_of(xyz, r, ok)
        P, idx, w, ijk = footprint(G, xyz, r, radius)
        status = taps(G, xyz, "radial", radius, None)[3]
        classes = (0, 2) if radius <= 0.5 else (0, 1, 2)  # (r <= 0.5: a footprint is one voxel at most, so none lands in part)
        assert all((status == s).any() for s in classes), f"{name} r={radius}: status classes {np.bincount(status, minlength=3).tolist()}"
        straddles = (((lo + E[:, None] - 1) >> 3) != (lo >> 3)).all(1) & ok
        assert radius < 1 or straddles.any(), f"{name} r={radius}: no box straddles eight leaves"
        x64 = xyz[ok].astype(np.float64)
        whole, shifted = x64 == np.floor(x64), (x64 - radius) == np.floor(x64 - radius)  # a voxel sits exactly r away along the shifted axes, on the point along the others
        n_shifted = shifted.sum(1)[(whole | shifted).all(1)]
        assert all((n_shifted == k).any() for k in (1, 2, 3)) or radius == np.floor(radius), f"{name} r={radius}: no voxel exactly r away along one, two and three axes"
        assert (n_shifted == 3).any()
        nf = np.bincount(P, minlength=len(xyz))
        assert nf.max() <= E.max() ** 3  # (the box bounds a footprint: 512 candidates at r = 4, of which some 280 lie within r)
        if radius == 0.5:
            centres = ok & (np.modf(np.abs(xyz))[0] == 0.5).all(1)
            assert centres.any()
    # an empty footprint: r = 0.4 at a cell centre
    centre = xyz[(np.modf(np.abs(xyz))[0] == 0.5).all(1) & finite & (np.abs(xyz) < 1e6).all(1)]
    assert len(centre) and len(footprint(G, centre, np.full(len(centre), F(0.4)), 4.0)[0]) == 0, f"{name}: r = 0.4 at a cell centre"


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    G = OracleGrid(case(name)[0])
    check_conditions(G, case(name)[3], name)
    return G


@functools.lru_cache(maxsize=None)
def cached_taps(name, kernel, radius, per_point):
    """`taps` of the whole point set of a grid, computed once per (kernel, radius)"""
    return taps(oracle_grid(name), case(name)[3], kernel, radius, case(name)[7] if per_point else None)


def mirror(grid, fields, xyz, values, log2_quantum=-32, masks=None, activate=True, **spec):
    """the host mirror under a spec, on copies -> (new fields, status, rejected, new masks or None)"""
    from hnanosolver_amd import api

    new = [np.array(f, dtype=F) for f in fields]
    m = None if masks is None else np.array(masks, dtype=np.uint8)
    status = np.full(len(xyz), 0xAB, dtype=np.uint8)
    rejected = api.splat_points_host(grid, new, xyz, values, log2_quantum, m, activate, status, **spec)
    return new, status, rejected, m


def spec_of(kernel, mode, radius=None, per_point=None, min_weight=0.0):
    """the keywords of the Python calls for a spec; per_point: one radius per point (then `radius` is their bound)"""
    kw = dict(kernel=kernel, mode=mode, min_weight=min_weight)
    if kernel == "radial":
        kw.update(radius=radius) if per_point is None else kw.update(radius=per_point, max_radius=radius)
    return kw
