"""CPU-side checks of the V-cycle pressure solve (include/hns.h: "A second solve method"), on its numpy mirror tests/mg_cases.py: the hierarchy's derivation against a
brute-force restatement, the convergence the method exists for, the failure mode its exact masks exist for, and the bookkeeping of the binding. The GPU tests
(tests/test_multigrid_gpu.py) hold the library against the same mirror in every word."""
import ctypes as C
import inspect

import numpy as np
import pytest

import mg_cases as mg
from hnanosolver_amd import _lib, device

RAGGED = dict(radius=4, drop=0.1, seed=11)  # 245 leaves of a ball of 64^3 extent with a tenth of its leaves knocked out


@pytest.mark.parametrize("name", sorted(mg.LEAF_SETS))
def test_hierarchy_matches_brute_force(name):
    """origins, masks, parent / octant / child tables of every level against the per-voxel restatement on global coordinates"""
    origins = mg.LEAF_SETS[name]()
    levels = mg.build_hierarchy(origins)
    assert levels[0].mask.all() and np.array_equal(levels[0].origins, origins)
    for fine, coarse in zip(levels[:-1], levels[1:]):
        want = mg.brute_force_level(fine.origins, fine.mask)
        assert sorted(want) == sorted(tuple(int(v) for v in o) for o in coarse.origins)
        assert coarse.n < fine.n
        for l, o in enumerate(coarse.origins):
            assert np.array_equal(coarse.mask[l], want[tuple(int(v) for v in o)]), f"{name}: mask of coarse leaf {o}"
            assert coarse.mask[l].any()
        for i, o in enumerate(fine.origins.astype(np.int64)):
            po = coarse.origins[fine.parent[i]].astype(np.int64)
            rel = o // 2 - po  # the leaf's corner voxel in its parent, in coarse voxels
            assert all(r in (0, 4) for r in rel) and fine.octant[i] == (rel[0] // 4) * 4 + (rel[1] // 4) * 2 + rel[2] // 4
            assert coarse.child[fine.parent[i], fine.octant[i]] == i
        assert (coarse.child >= 0).sum() == fine.n
    # the depth rule: the last level is one leaf, or coarsening it would not lower the leaf count
    last = levels[-1]
    assert last.n == 1 or len(mg.coarse_leaves(last.origins)[0]) >= last.n


def test_ragged_deep_has_partial_octants_at_level_two():
    """the set the list above was extended by. A level-1 mask is made of whole octants (4^3 voxels, one per fine leaf); on this set the masks of level 2 are not: some
    octant of a level-2 leaf holds unknowns and voxels that are none (2^3-voxel pieces, one per fine leaf), and level 3 goes down to single voxels"""
    levels = mg.build_hierarchy(mg.ragged_deep())
    assert len(levels) >= 4
    m1 = levels[1].mask.reshape(levels[1].n, 2, 4, 2, 4, 2, 4)
    assert (m1.all(axis=(2, 4, 6)) == m1.any(axis=(2, 4, 6))).all()
    for L in levels[2:]:
        m = L.mask.reshape(L.n, 2, 4, 2, 4, 2, 4)
        assert (m.any(axis=(2, 4, 6)) & ~m.all(axis=(2, 4, 6))).any()


def test_max_levels_and_single_leaf():
    o = mg.ragged_ball(**RAGGED)
    assert [L.n for L in mg.build_hierarchy(o, max_levels=2)] == [len(o), mg.build_hierarchy(o)[1].n]
    assert len(mg.build_hierarchy(o, max_levels=1)) == 1
    assert [L.n for L in mg.build_hierarchy(mg.LEAF_SETS["one_leaf"]())] == [1]


@pytest.fixture(scope="module")
def ragged_case():
    o = mg.ragged_ball(**RAGGED)
    div, vs = mg.flagship_divergence(o, 64)
    return o, div, vs


def test_converges_on_a_ragged_set(ragged_case):
    """max|c| after each of 6 V(2,2) cycles at omega = 1 is strictly below the one before, and after the sixth below 1e-2 of its value at p = 0. On this set and this
    right-hand side the mirror gives 1.9e-3 at p = 0, then 3.1e-4, 6.4e-5, 1.5e-5, 3.9e-6, 1.1e-6, 3.0e-7."""
    o, div, vs = ragged_case
    assert 200 <= len(o) <= 300
    h = mg.Mirror(o).history(div, vs, 6)
    print("ragged", h)
    assert all(b < a for a, b in zip(h[:-1], h[1:])), h
    assert h[6] < 1e-2 * h[0], h


def test_converges_on_the_dense_box():
    """the same on dense 32^3 (7.0e-3, then 8.5e-4, 1.3e-4, 2.5e-5, 5.5e-6, 1.1e-6, 2.7e-7)"""
    o = mg.LEAF_SETS["dense32"]()
    div, vs = mg.flagship_divergence(o, 32)
    h = mg.Mirror(o).history(div, vs, 6)
    print("dense32", h)
    assert all(b < a for a, b in zip(h[:-1], h[1:])), h
    assert h[6] < 1e-2 * h[0], h


def test_all_ones_masks_do_not_converge(ragged_case):
    """the failure mode the exact masks exist for: the same ragged set with every voxel of every coarse leaf an unknown must NOT satisfy the condition above (it grows:
    1.9e-3, 1.6e-3, 1.9e-3, 3.0e-3, 4.9e-3, 8.0e-3, 1.3e-2)"""
    o, div, vs = ragged_case
    h = mg.Mirror(o, exact_masks=False).history(div, vs, 6)
    print("all-ones", h)
    assert not mg.converges(h), h
    assert mg.converges(mg.Mirror(o).history(div, vs, 6))


def test_binding_and_defaults():
    assert C.sizeof(_lib.hns_solve_method) == 24
    assert [f[0] for f in _lib.hns_solve_method._fields_] == ["method", "pre", "post", "coarse_iterations", "max_levels", "omega"]
    assert _lib.SIGNATURES["hns_sim_set_solve_method"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.hns_solve_method)])
    assert _lib.SIGNATURES["hns_sim_solve_levels"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_int])
    d = {k: v.default for k, v in inspect.signature(device.Sim.solve_method).parameters.items() if k != "self"}
    assert d == {"method": 1, "pre": 2, "post": 2, "coarse_iterations": 8, "max_levels": 0, "omega": 1.0}  # V(2,2), 8 coarse iterations, omega 1.0
    # no stream parameter: the setter waits for its own device work, the solves keep their streams
    assert all(C.c_void_p not in args[1:] for args in (_lib.SIGNATURES["hns_sim_set_solve_method"][1], _lib.SIGNATURES["hns_sim_solve_levels"][1]))


def test_null_sim_is_refused():
    lib = _lib.load_library()
    m = _lib.hns_solve_method(1, 2, 2, 8, 0, 1.0)
    assert lib.hns_sim_set_solve_method(None, C.byref(m)) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert lib.hns_sim_set_solve_method(None, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    n = C.c_int(7)
    assert lib.hns_sim_solve_levels(None, C.byref(n), None, 0) == _lib.HNS_ERR_INVALID_ARGUMENT and n.value == 7
