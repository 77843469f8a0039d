"""CPU checks of the domain dilation that chains frames: hns_dilate_leaf_masks (the dilated active masks the next frame starts from) against a
dense brute force, the frame-to-frame growth it implies (SOP_HNanoSolver.cpp:186-199 with padding 1), and the bindings of the regrid ABI."""
import numpy as np
import pytest

from frame_cases import pack, unpack
from hnanosolver_amd import _lib, fields, leafio

PADDINGS = [0, 1, 3, 7, 8, 9, 17]


def brute_force(origins: np.ndarray, masks: np.ndarray, p: int):
    """Dense voxel bitmap of the leaves, dilated by p one-voxel shifts per axis (the Chebyshev ball is a box), cut back into leaves."""
    origins = np.asarray(origins, dtype=np.int64)
    lo = origins.min(0) - 8 * ((p + 7) // 8 + 1)
    hi = origins.max(0) + 8 + 8 * ((p + 7) // 8 + 1)
    ext = (hi - lo).astype(int)
    vol = np.zeros(ext, dtype=bool)
    bits = unpack(masks).reshape(-1, 8, 8, 8)
    for o, b in zip(origins - lo, bits):
        vol[o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8] |= b
    for axis in range(3):
        acc = vol.copy()
        for s in range(1, p + 1):
            acc |= np.roll(vol, s, axis) | np.roll(vol, -s, axis)  # the margin keeps the roll from wrapping anything set
        vol = acc
    leaves = vol.reshape(ext[0] // 8, 8, ext[1] // 8, 8, ext[2] // 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(ext[0] // 8, ext[1] // 8, ext[2] // 8, 512)
    keep = np.argwhere(leaves.any(-1))
    out = (keep * 8 + lo).astype(np.int32)
    return out, pack(leaves[tuple(keep.T)])


def random_case(seed: int):
    rng = np.random.default_rng(seed)
    o = np.unique(rng.integers(-5, 4, size=(14, 3)), axis=0).astype(np.int32) * 8
    o = np.concatenate([o, np.array([[160, -200, 96]], dtype=np.int32)])  # a lone leaf far from the rest
    o = o[rng.permutation(len(o))]  # not OpenVDB order
    bits = rng.random((len(o), 512)) < rng.choice([0.002, 0.02, 0.3], size=(len(o), 1))
    bits[0] = False  # an empty mask contributes nothing
    return o, pack(bits)


@pytest.mark.parametrize("p", PADDINGS)
def test_dilate_leaf_masks_against_brute_force(p):
    for seed in range(3):
        o, m = random_case(100 * p + seed)
        got_o, got_m = leafio.dilate_leaf_masks(o, p, m)
        assert np.array_equal(got_o, leafio.dilate_leaves(o, p, m)), "leaf set and order must be hns_dilate_leaves'"
        assert np.array_equal(got_o, got_o[fields.nanovdb_order(got_o)])
        want_o, want_m = brute_force(o, m, p)
        order = fields.nanovdb_order(want_o)
        assert np.array_equal(got_o, want_o[order])
        assert np.array_equal(got_m, want_m[order])


def test_dilate_leaf_masks_defaults_and_large_padding():
    o = np.array([[0, 0, 0], [-64, 8, 1024]], dtype=np.int32)
    full = np.full((2, 64), 0xFF, dtype=np.uint8)
    a = leafio.dilate_leaf_masks(o, 5)
    b = leafio.dilate_leaf_masks(o, 5, full)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = np.array([[8, -16, 24]], dtype=np.int32)
    centre = np.zeros((1, 512), dtype=bool)
    centre[0, (3 << 6) | (4 << 3) | 5] = True
    for p in (20, 64):
        got_o, got_m = leafio.dilate_leaf_masks(one, p, pack(centre))
        want_o, want_m = brute_force(one, pack(centre), p)
        order = fields.nanovdb_order(want_o)
        assert np.array_equal(got_o, want_o[order]) and np.array_equal(got_m, want_m[order])
    n, nm = leafio.dilate_leaf_masks(one, 200)  # every voxel of the leaf: ceil(200/8) leaves each way, the outermost ones partly covered
    assert len(n) == 51 ** 3 and np.array_equal(n, leafio.dilate_leaves(one, 200)) and (nm != 0).any(1).all()
    with pytest.raises(_lib.HNSError):
        leafio.dilate_leaf_masks(one, 1025)
    with pytest.raises(_lib.HNSError):
        leafio.dilate_leaf_masks(np.array([[4, 0, 0]], dtype=np.int32), 1)


def test_padding_one_grows_a_leaf_ring_every_eighth_frame():
    """The motivation, pinned: with padding 1 the active region grows one voxel a frame, so starting from full masks seven dilations in eight keep
    the leaf set -- because the masks carry the partial ring -- and the eighth adds a ring of leaves."""
    o = fields.dense_leaves(16)  # 2^3 leaves, every voxel active
    m = np.full((len(o), 64), 0xFF, dtype=np.uint8)
    counts = [len(o)]
    for _ in range(16):
        o, m = leafio.dilate_leaf_masks(o, 1, m)
        counts.append(len(o))
    assert counts == [8] + [64] + [64] * 7 + [216] + [216] * 7
    # without the masks (a host chain that only keeps leaves) every frame would add a ring
    assert len(leafio.dilate_leaves(fields.dense_leaves(16), 1)) == 64


def test_load_library_binds_the_regrid_symbols():
    lib = _lib.load_library()
    for name in ("hns_dilate_leaf_masks", "hns_sim_set_active_masks", "hns_sim_active_masks", "hns_sim_regrid", "hns_sim_regrid_times"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.hns_sim_regrid.restype is _lib.C.c_void_p
