"""The point sets of tests/test_points_gpu.py meet their conditions -- counted by the oracle, without a GPU: the shares of cells with all, some and none of their taps
inside, every point class present, and a traced set whose mirror shows points that leave the domain and stop and points that enter it."""
import numpy as np
import pytest

import points_cases as pc
from oracle_lib import OracleGrid


@pytest.mark.parametrize("name", [g for g in pc.GRIDS if g != "one_leaf"])
def test_shares_of_inside_partial_and_outside_cells(name):
    o, _, _, xyz = pc.case(name)
    full, part, none = pc.check_conditions(OracleGrid(o), xyz, name)
    print(f"{name}: all eight inside {full:.3f}, one to seven {part:.3f}, none {none:.3f}")


@pytest.mark.parametrize("name", pc.GRIDS)
def test_every_point_class_is_present(name):
    o, _, _, xyz = pc.case(name)
    assert xyz.shape == (pc.N_POINTS, 3) and xyz.dtype == np.float32 and np.isfinite(xyz).all()
    x64 = xyz.astype(np.float64)
    cell = np.floor(x64).astype(np.int64)
    on7 = ((cell & 7) == 7).sum(1)
    assert all((on7 == k).sum() >= 20 for k in (1, 2, 3)), "cells with the lower corner on local index 7 along one, two and three axes"
    assert ((x64 == cell).all(1)).sum() >= 100, "exact integer positions"
    below = np.nextafter(xyz, np.float32(np.inf)) == np.ceil(xyz)
    assert (below.any(1)).sum() >= 100 and (below & (xyz < 0)).any(), "positions an ulp below an integer, negative ones included"
    assert (np.abs(x64).max(1) > 2000).sum() >= 100 and np.abs(x64).max() > 2.0 ** 21 and np.abs(x64).max() <= 2.0 ** 22
    c = pc.taps_inside(OracleGrid(o), xyz)
    assert (c == 8).any() and ((c > 0) & (c < 8)).any() and (c == 0).any()
    for n in pc.COUNTS[1:]:  # every prefix the GPU test takes holds inside and outside cells from 63 points on
        assert n < 63 or ((c[:n] == 8).any() and (c[:n] == 0).any()), n


@pytest.mark.parametrize("speed", pc.SPEEDS)
@pytest.mark.parametrize("name", [g for g in pc.GRIDS if g != "one_leaf"])
def test_the_traced_set_leaves_stops_and_enters(name, speed):
    o, vel, _, xyz = pc.case(name)
    G = OracleGrid(o)
    for dt in (pc.DT, -pc.DT):
        u = pc.scaled_velocity(vel, speed, np.float32(dt) * np.float32(pc.INV_DX))
        path, status = pc.trace_mirror(G, u, xyz, dt, pc.INV_DX, 2, 3)
        inside0, inside3 = pc.leaf_exists(G, path[0]), status == 1
        left, entered = inside0 & ~inside3, ~inside0 & inside3
        stopped = ~pc.leaf_exists(G, path[2]) & (pc.taps_inside(G, path[2]) == 0) & (path[2] != path[0]).any(1)
        assert (path[3][stopped] == path[2][stopped]).all()
        print(f"{name} speed {speed} dt {dt}: left {left.sum()}, entered {entered.sum()}, moved out and stopped {stopped.sum()}")
        assert left.sum() >= 10, "points that leave the domain"
        assert speed < 1.0 or stopped.sum() >= 10, "points that leave the domain and stop (a step of half a voxel does not carry a point past every tap in two steps)"
        assert entered.sum() >= 10, "points that enter the domain"
