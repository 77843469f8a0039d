"""CPU checks of the diagnostics' host side: hns_leaf_stats against numpy (raw words of count / nan_count / min / max / max_abs; sum and sum_sq bit for
bit against a numpy restatement of the stated tree, and within the tree's derived error bound of math.fsum), closed forms of the residual's per-voxel
quantity c on the numpy restatement that the GPU tests compare the kernel with, and the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import diag_cases as dc
import frame_cases
import special_cases as sc
from hnanosolver_amd import _lib, api, fields, leafio

F = np.float32


def field_of(leaf_set, cls, ncomp, seed=0):
    n = len(sc.LEAF_SETS[leaf_set]())
    rng = np.random.default_rng([seed, sc.CLASSES.index(cls), ncomp, n])
    shape = (n * 512, 3) if ncomp == 3 else (n * 512,)
    return n, sc.plant(cls, rng.standard_normal(shape).astype(F), rng)


@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masks"])
@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("leaf_set", sorted(sc.LEAF_SETS))
def test_leaf_stats_equals_numpy(leaf_set, cls, masked, ncomp):
    n, v = field_of(leaf_set, cls, ncomp)
    masks = frame_cases.random_masks(11, n) if masked else None
    got = leafio.leaf_stats(v, masks)
    assert len(got) == ncomp
    depth = dc.tree_depth(n)
    for c in range(ncomp):
        comp = np.ascontiguousarray(v[:, c]) if ncomp == 3 else v
        want, t, t2 = dc.numpy_stats(comp, masks)
        assert got[c].tobytes() == want.tobytes(), f"component {c}: {got[c]} vs {want}"
        # the derived bound: every term passes through at most `depth` additions, each with relative error <= 2^-53
        for name, terms in (("sum", t), ("sum_sq", t2)):
            if np.isfinite(terms).all() and np.isfinite(got[c][name]):
                exact = math.fsum(terms.reshape(-1).tolist())
                bound = depth * 2.0 ** -53 * math.fsum(np.abs(terms).reshape(-1).tolist())
                assert abs(float(got[c][name]) - exact) <= bound, f"{name}: off by {abs(float(got[c][name]) - exact):.3e}, bound {bound:.3e}"


def test_leaf_stats_orders_signed_zeros_and_handles_nothing_left():
    v = np.zeros(512, dtype=F)
    v[5] = F(-0.0)
    r = leafio.leaf_stats(v)[0]
    assert r["min"].tobytes() == F(-0.0).tobytes() and r["max"].tobytes() == F(0.0).tobytes() and r["max_abs"].tobytes() == F(0.0).tobytes()
    v[:] = F(-0.0)
    r = leafio.leaf_stats(v)[0]
    assert r["min"].tobytes() == r["max"].tobytes() == F(-0.0).tobytes() and r["max_abs"].tobytes() == F(0.0).tobytes()
    assert r["sum"].tobytes() == np.float64(-0.0).tobytes() and r["sum_sq"].tobytes() == np.float64(0.0).tobytes()  # -0 + -0 = -0, (-0)^2 = +0
    for values, masks in ((np.full(1024, np.nan, dtype=F), None), (np.ones(1024, dtype=F), np.zeros((2, 64), dtype=np.uint8)), (np.zeros(0, dtype=F), None)):
        r = leafio.leaf_stats(values, masks)[0]
        assert (r["min"], r["max"]) == (np.inf, -np.inf) and r["max_abs"].tobytes() == F(0.0).tobytes()
        assert r["sum"].tobytes() == r["sum_sq"].tobytes() == np.float64(0.0).tobytes() and r["reserved"] == 0
        assert r["count"] == (1024 if masks is None and values.size else 0) and r["nan_count"] == r["count"]
    both = np.zeros(512, dtype=F)
    both[3], both[400] = np.inf, -np.inf  # +-inf are values: the sum is NaN, stored as the one quiet NaN the header names
    r = leafio.leaf_stats(both)[0]
    assert (r["min"], r["max"], r["max_abs"], r["sum_sq"]) == (-np.inf, np.inf, np.inf, np.inf) and r["sum"].tobytes() == np.uint64(0x7FF8000000000000).tobytes()


def test_two_calls_give_the_same_bytes_and_the_order_of_leaves_matters_only_as_stated():
    n, v = field_of("ragged32", "huge", 1)
    assert leafio.leaf_stats(v).tobytes() == leafio.leaf_stats(v.copy()).tobytes()


# ---- the residual's per-voxel quantity, on the numpy restatement ----


def dense(R):
    o = np.ascontiguousarray(fields.dense_leaves(R), dtype=np.int32)
    return o, fields.leaves_to_coords(o)


def test_residual_closed_form_zero_pressure():
    o = sc.LEAF_SETS["ragged32"]()
    rng = np.random.default_rng(1)
    div = rng.standard_normal(len(o) * 512).astype(F)
    dx = 0.1
    c = dc.residual_numpy(o, div, np.zeros_like(div), dx)
    assert np.array_equal(c, (-(div * (F(dx) * F(dx)))) * dc.INV6)  # p = 0: c = (-div dx^2) / 6


def test_residual_closed_form_unit_pressure_on_a_box():
    R = 16
    o, coords = dense(R)
    c = dc.residual_numpy(o, np.zeros(len(coords), dtype=F), np.ones(len(coords), dtype=F), 0.1)
    present = sum(((coords[:, a] > 0).astype(int) + (coords[:, a] < R - 1).astype(int)) for a in range(3))  # neighbours inside the box: 6, 5 (face), 4 (edge), 3 (corner)
    assert sorted(np.unique(present).tolist()) == [3, 4, 5, 6] and (present == 3).sum() == 8
    for m in (3, 4, 5, 6):
        want = F(F(m) * dc.INV6) - F(1.0)
        assert (c[present == m].view(np.uint32) == want.view(np.uint32)).all(), f"{m} neighbours: {np.unique(c[present == m])} vs {want}"
    assert len({c[present == m][0] for m in (3, 4, 5, 6)}) == 4  # faces, edges and corners each give their own value
    r = leafio.leaf_stats(c)[0]
    assert r["count"] == R ** 3 and r["min"] == F(F(3) * dc.INV6) - F(1.0) and r["max"] == 0.0


def test_residual_one_nan_reaches_itself_and_its_six_neighbours():
    R = 16
    o, coords = dense(R)
    rng = np.random.default_rng(2)
    p = rng.standard_normal(len(coords)).astype(F)
    at = np.flatnonzero((coords == [7, 3, 11]).all(axis=1))[0]  # on a leaf face: the +x neighbour lives in the next leaf
    p[at] = np.nan
    c = dc.residual_numpy(o, rng.standard_normal(len(coords)).astype(F), p, 0.05)
    hit = np.abs(coords - coords[at]).sum(axis=1) <= 1
    assert hit.sum() == 7 and np.array_equal(np.isnan(c), hit)
    r = leafio.leaf_stats(c)[0]
    assert r["nan_count"] == 7 and r["count"] == R ** 3 and np.isfinite(r["sum"])


# ---- refusals that need no device ----


def test_refusals_without_a_device():
    lib = _lib.load_library()
    out = (_lib.hns_stats * 3)()
    v = np.zeros(512, dtype=F)
    before = bytes(out)
    assert lib.hns_leaf_stats(1, None, v.ctypes.data, 2, out) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert lib.hns_leaf_stats(1, None, None, 1, out) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert lib.hns_leaf_stats(1, None, v.ctypes.data, 1, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    names = (_lib.hns_stats_field * 1)()
    names[0].name, names[0].ncomp = b"density", 1
    assert lib.hns_sim_stats(None, names, 1, 1, out, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert lib.hns_sim_residual(None, 0.1, out, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    ctl = _lib.hns_solve_control(1e-3, 0.0, 4)
    assert lib.hns_sim_set_solve_control(None, C.byref(ctl)) == _lib.HNS_ERR_INVALID_ARGUMENT
    rep = _lib.hns_solve_report()
    assert lib.hns_sim_solve_report(None, C.byref(rep), None, 0, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert bytes(out) == before
    g = api.create_grid_from_leaves(sc.LEAF_SETS["one_leaf"](), 0.1, _lib.HNS_GRID_HOST_ONLY)  # no device tables: no CPU fallback
    assert lib.hns_dev_residual(g.ptr, 8, 8, 0.1, None, 8, None) == _lib.HNS_ERR_NO_DEVICE
    assert lib.hns_dev_field_stats(g.ptr, 8, 1, None, 8, None) == _lib.HNS_ERR_NO_DEVICE
    assert lib.hns_dev_residual(None, 8, 8, 0.1, None, 8, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        leafio.leaf_stats(np.zeros(100, dtype=F))
