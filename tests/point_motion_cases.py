"""TEST HELPER of tests/test_point_motion_cases.py (CPU) and tests/test_point_motion_gpu.py: the inputs that points with a velocity of their own are stepped on, and the
mirror of k_move_points (hns_point_motion.hip) restated from the text of include/hns.h alone: numpy float32, one rounded operation per line, with S(x) the oracle's
sample_trilinear_f, U(x) its sample_trilinear_v on the fmaf branch of the Vec3f lerp, the cell and leaf rules of points_cases and the push of
points_collide_cases.push_out. Nothing here calls the library under test: the mirror is the oracle of every comparison, and the classes the conditions count are its own.

Inputs per grid of points_cases.GRIDS: the grid's velocity and its 4,099 points (points_cases.case), the lattice SDF (points_collide_cases.sdf_of), point velocities
3 * standard_normal and ages uniform(0, 1) from default_rng([7, GRIDS.index(name)])."""
from __future__ import annotations

import functools

import numpy as np

import points_cases as pc
import points_collide_cases as cc
from oracle_lib import OracleGrid

F = np.float32
MODES = ("free", "stick", "bounce", "kill")
HIT_BOUNCED, HIT_REVERTED, HIT_KILLED, HIT_START, HIT_REFLECTED = 1, 2, 4, 8, 16
DT, INV_DX, STEPS = 0.04, 24.0, 3
SPEC = dict(gravity=(0.0, -9.8, 0.0), drag=2.0, restitution=0.5, friction=0.25, threshold=0.0, skin=1.0 / 16, iterations=3, max_age=1.05)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(point velocities [4099, 3], ages [4099]) of a grid of points_cases.GRIDS: computed once, never written"""
    rng = np.random.default_rng([7, pc.GRIDS.index(name)])
    v = (3.0 * rng.standard_normal((pc.N_POINTS, 3))).astype(F)
    age = rng.uniform(0.0, 1.0, pc.N_POINTS).astype(F)
    v.setflags(write=False), age.setflags(write=False)
    return v, age


def motion_mirror(G, vel, sdf, xyz, v, age, dt, inv_dx, steps, mode, spec):
    """hns_point_motion_step restated. G: an OracleGrid, or None for a grid with no leaves (U = 0, S = 0, no leaf exists); sdf: None in mode "free", where S is never
    evaluated. -> (xyz, vel, age, status bytes, hit bytes, classes): classes is a dict of per-point counts of STEPS -- bounced; reflected (vn < 0); first_push /
    later_push: steps the first / a later push resolved; reverted: bounced steps put back after the last push"""
    assert mode in MODES
    sp = {**SPEC, **spec}
    one = F(1.0)
    # host constants
    dtf = F(dt)
    inv = F(inv_dx)
    s = dtf * inv
    k = F(sp["drag"]) * dtf
    r = one + k
    r = one / r
    gd = np.array([dtf * F(c) for c in sp["gravity"]], dtype=F)
    ft = one - F(sp["friction"])
    rest, thr, skin, max_age, iterations = F(sp["restitution"]), F(sp["threshold"]), F(sp["skin"]), F(sp["max_age"]), int(sp["iterations"])

    x = np.array(xyz, dtype=F).reshape(-1, 3)
    v = np.array(v, dtype=F).reshape(-1, 3)
    age = np.array(age, dtype=F).reshape(-1)
    n = len(x)

    def U(q):
        if G is None or not len(q):
            return np.zeros((len(q), 3), F)
        return np.array(G.sample_trilinear_v(vel, np.ascontiguousarray(q, dtype=F)), dtype=F)

    def S(q):
        if G is None or not len(q):
            return np.zeros(len(q), F)
        return np.array(G.sample_trilinear_f(sdf, np.ascontiguousarray(q, dtype=F)), dtype=F)

    hit = np.zeros(n, np.uint8)
    dead = np.zeros(n, bool)
    stepped = np.isfinite(x).all(1)  # Skip: the other rows keep every bit, status 0, hit 0
    cls = {c: np.zeros(n, np.int64) for c in ("bounced", "reflected", "first_push", "later_push", "reverted")}
    libs = (G.L,) if G is not None else ()
    with np.errstate(all="ignore"), pc.fma_branch(*libs) if libs else np.errstate():
        if mode != "free":
            start = np.zeros(n, bool)
            start[stepped] = S(x[stepped]) < thr
            hit[start] |= HIT_START
        for _ in range(steps):
            act = np.flatnonzero(stepped & ~dead)
            if not len(act):
                break
            x0 = x[act]
            u = U(x0)
            t = k * u
            t = v[act] + t
            v1 = t * r
            v1 = v1 + gd
            m = s * v1
            x1 = x0 + m
            a1 = age[act] + dtf
            killed = np.zeros(len(act), bool)
            if mode != "free":
                d = S(x1)
                coll = d < thr
                if mode == "stick":
                    x1[coll] = x0[coll]
                    v1[coll] = F(0.0)
                    hit[act[coll]] |= HIT_REVERTED
                elif mode == "kill":
                    hit[act[coll]] |= HIT_KILLED
                    killed = coll
                else:
                    hit[act[coll]] |= HIT_BOUNCED
                    cls["bounced"][act[coll]] += 1

                    def reflect(idx, nrm):  # the velocity, once a step
                        vv = v1[idx]
                        vn = vv[:, 0] * nrm[:, 0]
                        t2 = vv[:, 1] * nrm[:, 1]
                        vn = vn + t2
                        t2 = vv[:, 2] * nrm[:, 2]
                        vn = vn + t2
                        neg = vn < F(0.0)
                        w = vn[:, None] * nrm
                        vt = vv - w
                        a = rest * vn
                        pt = ft * vt
                        qn = a[:, None] * nrm
                        new = pt - qn
                        v1[idx[neg]] = new[neg]
                        hit[act[idx[neg]]] |= HIT_REFLECTED
                        cls["reflected"][act[idx[neg]]] += 1

                    first, later, inside = cc.push_out(S, x1, d, coll, thr, skin, inv, iterations, on_first=reflect)
                    cls["first_push"][act] += first
                    cls["later_push"][act] += later
                    cls["reverted"][act] += inside
                    rev = inside > 0
                    hit[act[rev]] |= HIT_REVERTED
                    x1[rev] = x0[rev]
            x[act], v[act], age[act] = x1, v1, a1
            dead[act[killed]] = True
    exists = pc.leaf_exists(G, x) if G is not None else np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        status = (stepped & ~dead & np.isfinite(x).all(1) & exists & (age < max_age)).astype(np.uint8)
    return x, v, age, status, hit, cls


def classes(x, age, status, hit, cls, max_age=SPEC["max_age"]):
    """the counts the conditions of tests/test_point_motion_cases.py are stated on: points, but for the outcomes of a bounced step, which are steps"""
    with np.errstate(invalid="ignore"):
        expired = np.isfinite(x).all(1) & ~(age < F(max_age))
    return {"start_in": int(((hit & HIT_START) != 0).sum()), "never_hit": int((hit == 0).sum()), "bounced": int(cls["bounced"].sum()),
            "reflected": int(cls["reflected"].sum()), "later_push": int(cls["later_push"].sum()), "reverted": int(cls["reverted"].sum()), "expired": int(expired.sum())}


@functools.lru_cache(maxsize=None)
def expected(name, variant, mode, dt=DT, steps=STEPS, inv_dx=INV_DX):
    """the mirror on the stated inputs of a grid: computed once, shared, never written"""
    o, vel, _, xyz = pc.case(name)
    v, age = inputs(name)
    out = motion_mirror(OracleGrid(o), vel, None if mode == "free" else cc.sdf_of(name, variant), xyz, v, age, dt, inv_dx, steps, mode, {})
    for a in out[:5]:
        a.setflags(write=False)
    return out
