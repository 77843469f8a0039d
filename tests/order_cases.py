"""TEST HELPER of tests/test_point_order.py (CPU) and tests/test_point_order_gpu.py: the leaf order of a point set restated in numpy from the text of include/hns.h
(never from the C++), the grids and the point sets the sort (hns_pointorder.hip, hns_grid_sort_points) is run on, and the conditions those sets must meet -- counted by
the restatement, never by the code under test.

The leaf order of a point set: a point sorts iff every coordinate c has -8388608.0f <= c < 8388607.0f (seed_cases.seeding); its cell is Floor; off is the grid's 1-based
offset of that voxel, 0 where its leaf is absent (the grid's `offsets`). Voxel key: off - 1, or 512 L for a sorting point whose leaf is absent, or 512 (L + 1) for a point that
does not sort. Level 1 sorts by the voxel key, level 0 by key >> 9; the sort is stable; keys[r] is the key of point perm[r]; leaf_start[q] = the number of points whose
leaf-level key is < q, q = 0 .. L + 2."""
from __future__ import annotations

import functools

import numpy as np

import points_cases as pc
import seed_cases as sd
import special_cases as sc
from hnanosolver_amd import _lib, api, fields

F = np.float32
VS = 1.0 / 24.0
LEVELS = (0, 1)
LEVEL_NAMES = {0: "leaf", 1: "voxel"}
GRIDS = ("ragged32", "ragged32_off_origin", "sparse_far", "dense32", "one_leaf", "dense64")  # dense64: fields.dense_leaves(64), the 512-leaf set
COUNTS = pc.COUNTS[:-1] + ("4099+edges",)
N_BIG = 70001  # the adversarial distributions: 34 tiles and a tail, no multiple of a wave


@functools.lru_cache(maxsize=None)
def origins(name):
    o = np.ascontiguousarray(fields.dense_leaves(64) if name == "dense64" else sc.LEAF_SETS[name](), dtype=np.int32)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def host_grid(name):
    """a host-only grid over the leaf set: what the restatement asks for offsets and the host mirror sorts on"""
    return api.create_grid_from_leaves(origins(name), VS, _lib.HNS_GRID_HOST_ONLY)


@functools.lru_cache(maxsize=None)
def full_set(name, n=pc.N_POINTS):
    """points_cases.make_points(origins, seed, n) followed by seed_cases.edges(): computed once, never written"""
    xyz = np.ascontiguousarray(np.concatenate([pc.make_points(origins(name), GRIDS.index(name), n), sd.edges()]), dtype=F)
    xyz.setflags(write=False)
    return xyz


def points(name, count):
    """the first `count` points of the grid's set; "4099+edges": all of it"""
    return full_set(name) if count == "4099+edges" else full_set(name)[:count]


def voxel_keys(grid, n_leaves, xyz):
    """the voxel key of every point, uint32"""
    x = np.asarray(xyz, dtype=F).reshape(-1, 3)
    sorts = sd.seeding(x)
    cell = np.floor(x[sorts].astype(np.float64)).astype(np.int32)  # exact in the sorting range
    off = grid.offsets(cell).astype(np.int64)
    key = np.full(len(x), 512 * (n_leaves + 1), dtype=np.int64)
    key[sorts] = np.where(off > 0, off - 1, 512 * n_leaves)
    assert key.max(initial=0) < 2 ** 32
    return key.astype(np.uint32)


def restate(grid, n_leaves, xyz, level):
    """-> (perm, keys, leaf_start), uint32, by the definition"""
    key = voxel_keys(grid, n_leaves, xyz)
    leaf_key = key >> 9
    k = key if level else leaf_key
    perm = np.argsort(k, kind="stable").astype(np.uint32)
    leaf_start = np.searchsorted(np.sort(leaf_key), np.arange(n_leaves + 3), side="left").astype(np.uint32)
    return perm, k[perm], leaf_start


def shares(grid, n_leaves, xyz):
    """(share of points in a leaf of the grid, share outside, number that do not sort), on the restatement's count"""
    leaf_key = voxel_keys(grid, n_leaves, xyz) >> 9
    n = max(1, len(leaf_key))
    return float((leaf_key < n_leaves).sum()) / n, float((leaf_key == n_leaves).sum()) / n, int((leaf_key == n_leaves + 1).sum())


def same(got, want, what=""):
    """two (perm, keys, leaf_start) triples as bytes; the message names the first array and entry that differ"""
    for name, g, w in zip(("perm", "keys", "leaf_start"), got, want):
        g, w = np.asarray(g).view(np.uint32).reshape(-1), np.asarray(w, dtype=np.uint32).reshape(-1)
        assert g.shape == w.shape, f"{what}: {name} has {g.shape} entries, expected {w.shape}"
        d = np.flatnonzero(g != w)
        assert len(d) == 0, f"{what}: {name} differs in {len(d)} of {g.size} entries, first at {d[:4].tolist()}: {g[d[:4]].tolist()} against {w[d[:4]].tolist()}"


def assert_stable_permutation(perm, keys, what=""):
    """stability stated directly: perm is a permutation of 0 .. n-1, keys do not decrease, and within every run of equal keys perm ascends"""
    perm, keys = np.asarray(perm).view(np.uint32).astype(np.int64), np.asarray(keys).view(np.uint32).astype(np.int64)
    n = len(perm)
    assert np.array_equal(np.sort(perm), np.arange(n)), f"{what}: perm is no permutation of 0 .. {n - 1}"
    assert (np.diff(keys) >= 0).all(), f"{what}: keys decrease"
    inside_run = np.diff(keys) == 0
    assert (np.diff(perm)[inside_run] > 0).all(), f"{what}: perm does not ascend within a run of equal keys"


# ---- adversarial distributions (about N_BIG points on a grid) -----------------------------------------------------------------------------------------------------------


def _in_leaf(o, leaf, local):
    return (np.asarray(o[leaf], dtype=np.float64) + np.asarray(local, dtype=np.float64)).astype(F)


def one_voxel(o, n=N_BIG):
    return np.ascontiguousarray(np.tile(_in_leaf(o, len(o) // 2, (3.25, 4.5, 5.75)), (n, 1)))


def alternating(o, n=N_BIG):
    """two keys in turn: a voxel of the last leaf, then one of the first"""
    two = np.stack([_in_leaf(o, len(o) - 1, (7.5, 0.25, 6.0)), _in_leaf(o, 0, (0.0, 7.99, 1.5))])
    return np.ascontiguousarray(two[np.arange(n) % 2])


def all_outside(o, n=N_BIG):
    return sd.emitter_ball(sd.outside_corner(o), seed=3, n=n)


def all_nan(o, n=N_BIG):
    return np.full((n, 3), np.nan, dtype=F)


def corner_ball(o, n=N_BIG):
    """an emitter ball on a leaf corner: up to eight leaves under one wave's points"""
    return sd.emitter_ball(np.asarray(o[len(o) // 2], dtype=np.float64) + 8.0, seed=5, n=n)


def mixed(o, n=N_BIG):
    return np.ascontiguousarray(np.concatenate([pc.make_points(o, 11, n - len(sd.edges())), sd.edges()]), dtype=F)


def ordered(grid, o, n=N_BIG, reverse=False):
    """`mixed` already in voxel order, or in the reverse of it"""
    x = mixed(o, n)
    perm = restate(grid, len(o), x, 1)[0]
    return np.ascontiguousarray(x[perm[::-1] if reverse else perm])


DISTRIBUTIONS = ("one_voxel", "sorted", "reversed", "alternating", "all_outside", "all_nan", "corner_ball")


@functools.lru_cache(maxsize=None)
def distribution(kind, grid_name="dense64"):
    o, g = origins(grid_name), host_grid(grid_name)
    xyz = {"one_voxel": lambda: one_voxel(o), "sorted": lambda: ordered(g, o), "reversed": lambda: ordered(g, o, reverse=True), "alternating": lambda: alternating(o),
           "all_outside": lambda: all_outside(o), "all_nan": lambda: all_nan(o), "corner_ball": lambda: corner_ball(o)}[kind]()
    xyz = np.ascontiguousarray(xyz, dtype=F)
    xyz.setflags(write=False)
    return xyz
