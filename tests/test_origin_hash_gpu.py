"""The origin hash (hnanosolver_amd/csrc/hns_originhash.hpp) where no other test takes it: probes that run past a table's last slot and wrap, and a duplicate or an
absent key at the far end of a collision chain -- for a grid's index table (k_hash_insert, d_find_leaf), a source's (k_regrid_src_hash, find_origin), a point set's key
table (k_seed_keys) and the regrid's candidate table (k_regrid_candidates). Every input set is SEARCHED for among the leaves of a small box with the numpy restatement
of hash_origin (tests/grid_cases.py), and the property it is used for -- at least two keys whose home slot is the table's last slot, so that a probe wraps whatever the
insertion order -- is asserted before it is used. Every comparison is on bytes, against the host builder or the host chain."""
import numpy as np
import pytest

import seed_cases as sd
from frame_cases import COMBUST, assert_same, download, host_chain, make_sim, random_state
from grid_cases import assert_device_tables_match_host_builder, box_leaves, home_slots
from hnanosolver_amd import _lib, api, device, leafio
from test_sources_gpu import raw_regrid

pytestmark = pytest.mark.gpu

F = np.float32
BOX = box_leaves()  # leaf coordinates in [-6, 6)^3


def at_last_slot(origins, slots):
    """those of `origins` whose home slot is the last of a table of `slots` slots"""
    origins = np.asarray(origins, dtype=np.int32)
    return origins[home_slots(origins, slots) == slots - 1]


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


# ---- a grid's index table: 7 leaves, 2 * 7 + 2 = 16 slots ------------------------------------------------------------------------------------------------------------------


def test_grid_table_with_every_leaf_at_the_last_slot():
    chain = at_last_slot(BOX, 16)
    assert len(chain) >= 9, "the box holds seven leaves for the grid and two absent origins of the same home slot"
    o = np.ascontiguousarray(chain[np.random.default_rng(1).permutation(7)])  # caller order
    absent = chain[7:]
    assert (home_slots(o, 16) == 15).all() and (home_slots(absent, 16) == 15).all()
    assert_device_tables_match_host_builder(o)
    g = api.create_grid_from_leaves(o, 0.1)
    h = api.create_grid_from_leaves(o, 0.1, _lib.HNS_GRID_HOST_ONLY)
    probes = np.ascontiguousarray(np.concatenate([absent, absent + 7]))  # the first and the last voxel of every absent leaf: a probe that walks the whole chain and ends on an empty slot
    assert not g.offsets(probes).any() and not h.offsets(probes).any()
    assert np.array_equal(g.offsets(o), np.arange(7, dtype=np.uint64) * 512 + 1) and np.array_equal(h.offsets(o), g.offsets(o))
    g.reset(), h.reset()
    o[-1] = o[0]
    for flags in (0, _lib.HNS_GRID_HOST_ONLY):
        with pytest.raises(api.HNSError, match="appears twice"):
            api.create_grid_from_leaves(o, 0.1, flags)


# ---- a source's index table: 8 leaves, 16 slots ----------------------------------------------------------------------------------------------------------------------------


def source_case():
    """a dense sim of 2^3 leaves placed where it holds the most leaves of home slot 15 of 16, and two sets of eight such leaves, inside the sim's domain and outside it"""
    chain = at_last_slot(BOX, 16)
    block = box_leaves(0, 2)
    best = max((b for b in BOX.tolist()), key=lambda b: len(at_last_slot(np.array(b, dtype=np.int32) + block, 16)))
    domain = (np.array(best, dtype=np.int32) + block).astype(np.int32)
    inside = at_last_slot(domain, 16)
    outside = np.array([c for c in chain.tolist() if c not in inside.tolist()], dtype=np.int32)
    assert 1 <= len(inside) <= 6 and len(outside) >= 16 - len(inside)
    k = 8 - len(inside)
    rng = np.random.default_rng(2)
    sets = [np.concatenate([inside, outside[:k]]), np.concatenate([outside[k:2 * k], inside])]
    sets = [np.ascontiguousarray(s[rng.permutation(8)]) for s in sets]
    for s in sets:
        assert len(np.unique(s, axis=0)) == 8 and (home_slots(s, 16) == 15).all()
    return domain, sets


def test_source_tables_with_every_leaf_at_the_last_slot():
    names = COMBUST
    o, (fo, vo) = source_case()
    st = random_state(3, len(o), names)
    rng = np.random.default_rng(4)
    src = {"density": (fo, None, rng.standard_normal(8 * 512).astype(F)), "vel": (vo, None, rng.standard_normal((8 * 512, 3)).astype(F))}
    g, s = make_sim(o, names, st)
    ng = s.regrid(1, None, src)
    dom, dm, want = host_chain(o, None, st, names, 1, src)
    assert np.array_equal(ng.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "sources at the last slot")
    s.close()
    # the last origin once more, in the slot before it: still eight leaves and 16 slots, the duplicate at the far end of the chain
    g, s = make_sim(o, names, st)
    for name, nc, so in (("density", 1, fo), ("vel", 3, vo)):
        d = so.copy()
        d[-2] = d[-1]
        v = np.ones((8 * 512, 3) if nc == 3 else 8 * 512, dtype=F)
        ptr, err, text = raw_regrid(s, 1, [(name, nc, d, None, v, 8)])
        assert not ptr and err == _lib.HNS_ERR_TOPOLOGY and "duplicate leaf origin" in text, (name, err, text)
        assert s.grid is g and np.array_equal(g.coords()[::512], o)
        assert_same(download(s, names), st, "after the refusal")
    s.close()


# ---- a point set's key table: one point, 8 leaves, 16 slots ----------------------------------------------------------------------------------------------------------------


def seed_cell():
    """the lower leaf of the first 2 x 2 x 2 leaves of the box of which two or more have home slot 15 of 16, and those eight leaves"""
    block = box_leaves(0, 2)
    for b in BOX:
        if len(at_last_slot(b + block, 16)) >= 2:
            return b, (b + block).astype(np.int32)
    raise AssertionError("no such cell in the box")


def test_seed_keys_that_collide_at_the_last_slot():
    lower, leaves = seed_cell()
    assert (home_slots(leaves, 16) == 15).sum() >= 2
    corner = (lower.astype(np.float64) + 7.5).astype(F).reshape(1, 3)  # the top corner voxel of the lower leaf: its cell has a tap in each of the eight leaves
    want = leafio.point_leaves(corner)
    assert len(want[0]) == 8 and sorted(want[0].tolist()) == sorted(leaves.tolist())
    assert sd.same(device.point_leaves(dev(corner)), want), "one point"
    copies = np.ascontiguousarray(np.repeat(corner, 64, axis=0))
    assert sd.same(device.point_leaves(dev(copies)), leafio.point_leaves(copies)), "64 copies: one wave, one key per leaf"
    rng = np.random.default_rng(5)
    spread = (leaves[np.arange(64) % 8].astype(np.float64) + rng.integers(0, 7, (64, 3)) + 0.25).astype(F)  # cells inside one leaf each, eight points per leaf
    spread = np.ascontiguousarray(spread[rng.permutation(64)])
    want = leafio.point_leaves(spread)
    assert sorted(want[0].tolist()) == sorted(leaves.tolist())
    assert sd.same(device.point_leaves(dev(spread)), want), "64 points over the eight leaves"


# ---- the candidate table: one leaf, padding within a leaf, 27 candidates, 64 slots -------------------------------------------------------------------------------------------


def candidate_leaf():
    """the first leaf of the box of whose 27 candidates two or more have home slot 63 of 64"""
    around = box_leaves(-1, 2)
    for b in BOX:
        if len(at_last_slot(b + around, 64)) >= 2:
            return np.ascontiguousarray(b.reshape(1, 3))
    raise AssertionError("no such leaf in the box")


@pytest.mark.parametrize("p", [1, 8])
def test_candidates_that_collide_at_the_last_slot(p):
    names = COMBUST
    o = candidate_leaf()
    assert (home_slots(o + box_leaves(-1, 2), 64) == 63).sum() >= 2
    st = random_state(6, 1, names)
    g, s = make_sim(o, names, st)  # all voxels active: each of the 27 candidates is reached
    ng = s.regrid(p)
    dom, dm, want = host_chain(o, None, st, names, p)
    assert len(dom) == 27
    assert np.array_equal(ng.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"p={p}")
    s.close()
