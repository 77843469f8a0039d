"""Conditions on the mirror of hns_point_motion_step (tests/point_motion_cases.py) alone, without a GPU: the inputs of the GPU comparison of tests/test_point_motion_gpu.py
meet every branch of the arithmetic often enough that equality with the mirror cannot be trivially green, and the mirror gives the answers that follow from the text of
include/hns.h by hand."""
import numpy as np
import pytest

import point_motion_cases as mc
import points_cases as pc
import points_collide_cases as cc
from oracle_lib import OracleGrid

F = np.float32
# points that start inside, points never hit, bounced steps, reflected steps (vn < 0), steps a later push resolved, steps put back, points expired
BOUNDS = {"start_in": 400, "never_hit": 1000, "bounced": 500, "reflected": 250, "later_push": 100, "reverted": 40, "expired": 100}


def bits(a):
    return np.ascontiguousarray(a, dtype=F).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("name,share", [("ragged32", 1.0), ("sparse_far", 0.2), ("one_leaf", 0.2)])
def test_the_bounce_inputs_meet_every_branch(name, share):
    x, v, age, status, hit, cls = mc.expected(name, "full", "bounce")
    c = mc.classes(x, age, status, hit, cls)
    print(name, c)
    for k, bound in BOUNDS.items():
        assert c[k] >= bound * share, f"{name}: {k} {c[k]} is below {bound * share}: {c}"
    assert not np.isnan(x).any() and not np.isnan(v).any() and not np.isnan(age).any()
    assert status.sum() >= 100 and (status == 0).sum() >= 100


def test_every_mode_differs_and_the_flags_are_the_modes():
    out = {m: mc.expected("ragged32", "full", m) for m in mc.MODES}
    assert not out["free"][4].any()
    assert set(np.unique(out["stick"][4] & ~np.uint8(mc.HIT_START))) == {0, mc.HIT_REVERTED}
    assert set(np.unique(out["kill"][4] & ~np.uint8(mc.HIT_START))) == {0, mc.HIT_KILLED}
    assert (out["bounce"][4] & mc.HIT_REFLECTED).astype(bool).sum() >= 250
    assert not (out["kill"][3][(out["kill"][4] & mc.HIT_KILLED) != 0]).any(), "a killed point has status 0"
    for a, b in (("free", "stick"), ("stick", "bounce"), ("bounce", "kill")):
        assert (bits(out[a][0]) != bits(out[b][0])).any()


def one_leaf():
    o = pc.case("one_leaf")[0]
    G = OracleGrid(o)
    return o, G, np.asarray(G.coords(), dtype=np.int64)


def test_without_drag_and_gravity_a_free_point_moves_in_a_straight_line():
    """drag 0, gravity 0, FREE: k = 0, r = 1, gd = 0, so v = (v + 0*u) * 1 + 0 and x1 = x + s*v"""
    o, vel, _, xyz = pc.case("ragged32")
    v, age = mc.inputs("ragged32")
    x1, v1, a1, status, hit, _ = mc.motion_mirror(OracleGrid(o), vel, None, xyz, v, age, mc.DT, mc.INV_DX, 1, "free", dict(drag=0.0, gravity=(0, 0, 0)))
    s = F(mc.DT) * F(mc.INV_DX)
    m = s * v
    assert np.array_equal(bits(x1), bits(xyz + m)) and np.array_equal(v1, v) and np.array_equal(bits(a1), bits(age + F(mc.DT))) and not hit.any()


def test_a_point_at_rest_on_a_positive_sdf_is_a_free_point_in_every_mode():
    o, G, c = one_leaf()
    sdf = np.full(len(c), 0.25, F)
    vel = np.zeros((len(c), 3), F)
    x = (c[0] + np.array([[3.25, 4.5, 2.75], [1.5, 1.5, 6.25]])).astype(F)
    v, age = np.zeros((2, 3), F), np.array([0.25, 0.5], F)
    free = mc.motion_mirror(G, vel, None, x, v, age, 0.04, 24.0, 3, "free", dict(gravity=(0, 0, 0)))
    assert np.array_equal(bits(free[0]), bits(x)) and np.array_equal(bits(free[2]), bits((age + F(0.04) + F(0.04)) + F(0.04))) and free[3].all()
    for mode in ("stick", "bounce", "kill"):
        got = mc.motion_mirror(G, vel, sdf, x, v, age, 0.04, 24.0, 3, mode, dict(gravity=(0, 0, 0)))
        for a, b in zip(got[:5], free[:5]):
            assert np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b), mode
    # ... and moving points against a positive SDF, whatever the mode
    o, vel, _, xyz = pc.case("ragged32")
    v, age = mc.inputs("ragged32")
    positive = np.abs(cc.sdf_of("ragged32", "full")) + F(0.01)
    free = mc.expected("ragged32", "full", "free")
    for mode in ("stick", "bounce", "kill"):
        got = mc.motion_mirror(OracleGrid(o), vel, positive, xyz, v, age, mc.DT, mc.INV_DX, mc.STEPS, mode, {})
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], free[:3])) and np.array_equal(got[3], free[3]) and not got[4].any(), mode


def test_normal_incidence_on_a_plane_flips_the_normal_velocity_exactly():
    """sdf = (y - 4) / 8 at inv_dx = 8: the central difference is (0, 1, 0) exactly. restitution 1, friction 0, no drag, no gravity, s = dt * inv_dx = 1: the point falls from
    y = 4.5 to 3.5 (d = -1/16), v.y = -1 becomes +1, and the push lifts it by (0 - d) * 8 + 1/16 to 4.0625"""
    o, G, c = one_leaf()
    sdf = ((c[:, 1] - c[0, 1] - 4) * 0.125).astype(F)
    vel = np.zeros((len(c), 3), F)
    x = (c[0] + np.array([[3.5, 4.5, 3.5]])).astype(F)
    v, age = np.array([[0.0, -1.0, 0.0]], F), np.zeros(1, F)
    spec = dict(drag=0.0, gravity=(0, 0, 0), restitution=1.0, friction=0.0, max_age=np.inf)
    x1, v1, a1, status, hit, cls = mc.motion_mirror(G, vel, sdf, x, v, age, 0.125, 8.0, 1, "bounce", spec)
    assert v1.tolist() == [[0.0, 1.0, 0.0]] and (x1 - c[0]).tolist() == [[3.5, 4.0625, 3.5]]
    assert hit.tolist() == [mc.HIT_BOUNCED | mc.HIT_REFLECTED] and status.tolist() == [1] and a1.tolist() == [0.125]
    # restitution 0.5 and friction 0.25 on oblique incidence: the normal part halves and turns, the tangential part loses a quarter
    v = np.array([[2.0, -1.0, -4.0]], F)
    x = (c[0] + np.array([[1.5, 4.5, 7.5]])).astype(F)  # lands at (3.5, 3.5, 3.5)
    _, v1, _, _, hit, _ = mc.motion_mirror(G, vel, sdf, x, v, age, 0.125, 8.0, 1, "bounce", {**spec, "restitution": 0.5, "friction": 0.25})
    assert v1.tolist() == [[1.5, 0.5, -3.0]] and hit.tolist() == [mc.HIT_BOUNCED | mc.HIT_REFLECTED]
    # a point that leaves the collider is pushed but not reflected
    v = np.array([[0.0, 0.25, 0.0]], F)
    x = (c[0] + np.array([[3.5, 3.0, 3.5]])).astype(F)
    _, v1, _, _, hit, _ = mc.motion_mirror(G, vel, sdf, x, v, age, 0.125, 8.0, 1, "bounce", spec)
    assert v1.tolist() == [[0.0, 0.25, 0.0]] and hit.tolist() == [mc.HIT_BOUNCED | mc.HIT_START]


def test_stick_puts_the_point_back_with_zero_velocity_and_kill_freezes_it():
    o, vel, _, xyz = pc.case("ragged32")
    v, age = mc.inputs("ragged32")
    x1, v1, a1, status, hit, _ = mc.motion_mirror(OracleGrid(o), vel, cc.sdf_of("ragged32", "full"), xyz, v, age, mc.DT, mc.INV_DX, 1, "stick", {})
    stuck = (hit & mc.HIT_REVERTED) != 0
    assert stuck.sum() >= 100 and not bits(v1[stuck]).any() and np.array_equal(bits(x1[stuck]), bits(xyz[stuck])) and (x1[~stuck] != xyz[~stuck]).any(1).all()
    assert np.array_equal(bits(a1), bits(age + F(mc.DT)))
    # kill: the state after one step is the state after three for a point the first step killed
    k1 = mc.motion_mirror(OracleGrid(o), vel, cc.sdf_of("ragged32", "full"), xyz, v, age, mc.DT, mc.INV_DX, 1, "kill", {})
    k3 = mc.expected("ragged32", "full", "kill")
    killed = (k1[4] & mc.HIT_KILLED) != 0
    assert killed.sum() >= 100 and all(np.array_equal(bits(a[killed]), bits(b[killed])) for a, b in zip(k1[:3], k3[:3])) and not k3[3][killed].any()


@pytest.mark.parametrize("mode", mc.MODES)
def test_a_row_without_a_position_keeps_every_bit(mode):
    o, vel, _, xyz = pc.case("one_leaf")
    v, age = mc.inputs("one_leaf")
    x = np.array(xyz[:64])
    x[::4, 0] = np.nan
    x[1::8, 2] = np.inf
    x[2::8, 1] = -np.inf
    gone = ~np.isfinite(x).all(1)
    got = mc.motion_mirror(OracleGrid(o), vel, None if mode == "free" else cc.sdf_of("one_leaf", "full"), x, v[:64], age[:64], mc.DT, mc.INV_DX, 2, mode, {})
    assert np.array_equal(bits(got[0][gone]), bits(x[gone])) and np.array_equal(bits(got[1][gone]), bits(v[:64][gone])) and np.array_equal(bits(got[2][gone]), bits(age[:64][gone]))
    assert not got[3][gone].any() and not got[4][gone].any()
    want = mc.motion_mirror(OracleGrid(o), vel, None if mode == "free" else cc.sdf_of("one_leaf", "full"), xyz[:64], v[:64], age[:64], mc.DT, mc.INV_DX, 2, mode, {})
    assert all(np.array_equal(a[~gone], b[~gone]) for a, b in zip(got[:5], want[:5])), "rows are independent"


def test_a_grid_without_leaves_lets_points_fall():
    """U = 0, S = 0, no leaf exists: v = (v + 0) * r + gd, every status 0, and against threshold 0 nothing is in collision"""
    v, age = mc.inputs("one_leaf")
    xyz = pc.case("one_leaf")[3][:65]
    x1, v1, a1, status, hit, _ = mc.motion_mirror(None, None, None, xyz, v[:65], age[:65], mc.DT, mc.INV_DX, 1, "bounce", {})
    k = F(2.0) * F(mc.DT)
    r = F(1.0) / (F(1.0) + k)
    want_v = (v[:65] + F(0.0)) * r + np.array([0, F(mc.DT) * F(-9.8), 0], F)
    assert np.array_equal(bits(v1), bits(want_v)) and np.array_equal(bits(x1), bits(xyz + (F(mc.DT) * F(mc.INV_DX)) * want_v)) and not status.any() and not hit.any()
