"""The inputs of tests/test_points_collide_gpu.py, checked without a GPU: on the mirror of tests/points_collide_cases.py (the oracle's samplers, never the library under
test) every combination of grid, SDF variant, speed, sign of dt and order, at 3 steps, threshold 0, skin 1/16 and 3 iterations, holds enough points of every class the
kernel treats differently: points that start in collision, points that never touch anything, reverted and killed points, pushes resolved by the first push, by a later
one and by none, and pushed points that end in another leaf than they started in."""
import numpy as np
import pytest

import points_cases as pc
import points_collide_cases as cc
from oracle_lib import OracleGrid

F = np.float32
STEPS = 3


def test_the_lattice_sdf_is_the_closed_form():
    o = pc.case("dense32")[0]
    G = OracleGrid(o)
    c = G.coords().astype(np.int64)
    s = cc.sdf_of("dense32", "full")
    assert s.dtype == F and s.shape == (len(o) * 512,)
    corner = (c % 8 == 0).all(1)
    assert (s[corner] == F(-3.0 / 24.0)).all() and corner.sum() == len(o)  # a sphere's centre on every leaf corner
    assert (s[((c % 8) == 4).all(1)] == F((np.sqrt(48.0) - 3.0) / 24.0)).all()
    inside = float((s < 0).mean())
    assert 0.15 < inside < 0.30, inside  # (the continuous share is 4/3 pi 27 / 512 = 0.22)
    b = cc.sdf_of("dense32", "banded")
    band = np.abs(s) <= F(2.0 / 24.0)
    assert (b[band] == s[band]).all() and (b[~band].view(np.uint32) == 0x01010101).all() and 0.1 < (~band).mean() < 0.9
    assert ((b < 0) == ((s < 0) & band)).all()


@pytest.mark.parametrize("variant", cc.VARIANTS)
@pytest.mark.parametrize("name", pc.GRIDS)
def test_every_combination_holds_every_class(name, variant):
    o, vel, _, xyz = pc.case(name)
    G, sdf = OracleGrid(o), cc.sdf_of(name, variant)
    low = {}
    for speed in pc.SPEEDS:
        for dt in (pc.DT, -pc.DT):
            u = pc.scaled_velocity(vel, speed, F(dt) * F(pc.INV_DX))
            for order in (1, 2, 4):
                what = f"{name} {variant} speed {speed} dt {dt} order {order}"
                c = {}
                for mode in cc.MODES:
                    got, status, hit, cls = cc.collide_mirror(G, u, sdf, xyz, dt, pc.INV_DX, order, STEPS, mode)
                    c[mode] = cc.classes(xyz, got, hit, cls)
                    assert c[mode]["start_in"] >= 500 and c[mode]["never_hit"] >= 2000, f"{what} {mode}: {c[mode]}"
                    assert ((hit & cc.HIT_KILLED) == 0).all() or mode == "kill"
                    assert (status[(hit & cc.HIT_KILLED) != 0] == 0).all()
                assert c["stop"]["reverted"] >= 50, f"{what}: {c['stop']}"
                assert c["kill"]["killed"] >= 50, f"{what}: {c['kill']}"
                p = c["push"]
                assert p["first_push"] >= 30 and p["later_push"] >= 20 and p["push_reverted"] >= 10 and p["pushed_other_leaf"] >= 50, f"{what}: {p}"
                for mode in cc.MODES:
                    for k, v in c[mode].items():
                        low[mode, k] = min(low.get((mode, k), v), v)
    print(f"{name} {variant}: minima over speeds, signs and orders: { {f'{m} {k}': v for (m, k), v in low.items() if v} }")
