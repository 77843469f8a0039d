"""Point values into fields through a leaf order, without a GPU: the conditions tests/binned_cases.py sets for the point sets the GPU test runs (asserted from the numpy
restatements alone), the argument handling of device.PointOrder.splat and device.Sim.splat(order=...) that needs no device, and the two prototypes in _lib.py."""
import ctypes as C

import numpy as np
import pytest

import binned_cases as bc
from hnanosolver_amd import _lib, device

BAD = _lib.HNS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", bc.GRIDS)
def test_the_cases_carry_what_can_go_wrong(name):
    bc.check_conditions(name)


@pytest.mark.parametrize("name", bc.GRIDS)
def test_the_planted_points_are_a_binned_point_and_a_tail_point(name):
    import splat_cases as sp

    ok, leaf = bc.binned(sp.oracle_grid(name), bc.case(name)["xyz"][: bc.N_PLANTED])
    assert ok.tolist() == [True, False] and leaf[0] >= 0
    for kind in bc.KINDS:
        c = bc.case(name, kind)
        n = len(c["xyz"])
        assert n > max(k for k in bc.COUNTS if k != "all") and all(len(v) == n for v in c["vals"]) and len(c["vvals"]) == n
        assert (kind == "trilinear" and c["radii"] is None) or (kind == "radial" and len(c["radii"]) == n)


def test_both_prototypes_bind():
    lib = _lib.load_library()
    assert lib.hns_point_order_splat.restype is C.c_int and len(lib.hns_point_order_splat.argtypes) == 10
    assert lib.hns_point_order_splat_sim.restype is C.c_int and len(lib.hns_point_order_splat_sim.argtypes) == 12
    # a null object is refused by name, with or without a device
    one, ptrs = (C.c_int * 1)(1), (C.c_void_p * 1)(None)
    assert lib.hns_point_order_splat(None, ptrs, one, 1, None, ptrs, 0, -32, None, None) == BAD
    assert lib.hns_last_error().decode().startswith("hns_point_order_splat: null point order")
    assert lib.hns_point_order_splat_sim(None, None, None, 0, None, None, ptrs, 0, -32, 1, None, None) == BAD
    assert lib.hns_last_error().decode().startswith("hns_point_order_splat_sim: null point order")


def bare_order(n, level="voxel"):
    """a PointOrder as the wrappers see it after a sort of n points, without the library object behind it (which needs a device)"""
    o = object.__new__(device.PointOrder)
    o.grid, o.capacity, o._sim, o._ptr, o.n, o.level = None, n, None, 0, n, level
    return o


def test_the_wrappers_check_their_arguments_before_the_library_is_called():
    import torch

    n = 5
    xyz, v, st = torch.zeros((n, 3)), torch.zeros(n), torch.zeros(n, dtype=torch.uint8)
    o = bare_order(n)
    assert device.SPLAT_ROWS == {"original": 0, "ranked": 1}
    assert o._splat_rows("PointOrder.splat", "original", xyz, [("values[0]", v), ("status", st)]) == 0 and o._splat_rows("PointOrder.splat", "ranked", xyz, [("status", None)]) == 1
    for bad in ("sorted", 0, 1, None):
        with pytest.raises(ValueError, match="rows must be"):
            o.splat([v], xyz, [v], rows=bad)
    with pytest.raises(RuntimeError, match="no sort has run"):
        bare_order(n, level=None).splat([v], xyz, [v])
    with pytest.raises(ValueError, match=r"\(n, 3\) float32"):
        o.splat([v], xyz.reshape(-1), [v])
    with pytest.raises(ValueError, match=r"\(n, 3\) float32"):
        o.splat([v], xyz.double(), [v])
    with pytest.raises(ValueError, match="xyz has 4 rows, the last sort 5"):
        o.splat([v], xyz[:4], [v])
    with pytest.raises(ValueError, match=r"values\[0\] has 4 rows"):
        o.splat([v], xyz, [v[:4]])
    with pytest.raises(ValueError, match="status has 6 rows"):
        o.splat([v], xyz, [v], status=torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="closed"):  # every check passed: the call would go to the library now
        o.splat([v], xyz, [v])

    s = object.__new__(device.Sim)
    s.grid, s.names, s._ptr = None, ["density"], 0
    with pytest.raises(ValueError, match="pass no stream"):
        s.splat({"density": v}, xyz, order=o, stream=0)
    with pytest.raises(ValueError, match="rows must be"):
        s.splat({"density": v}, xyz, order=o, rows="both")
    with pytest.raises(ValueError, match="density has 4 rows"):
        s.splat({"density": v[:4]}, xyz, order=o)
    with pytest.raises(ValueError, match="velocity has 4 rows"):
        s.splat({"density": v}, xyz, velocity=xyz[:4], order=o)
    with pytest.raises(ValueError, match="rows is about an order"):
        s.splat({"density": v}, xyz, rows="ranked")
    other = bare_order(n)
    other.grid = object()
    with pytest.raises(ValueError, match="another grid"):
        s.splat({"density": v}, xyz, order=other)
    s._ptr = 0  # (nothing to close)
