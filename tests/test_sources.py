"""CPU checks of compSum over raw leaf sets (hns_add_leaves, the host mirror of hns_sim_regrid_sourced's sum) against a dense numpy brute force,
and the bindings of the sourced regrid ABI."""
import numpy as np
import pytest

from frame_cases import pack, unpack
from hnanosolver_amd import _lib, fields, leafio


def brute_force(a, b, ncomp):
    """Both sides painted into one dense box (values default +0.0f, masks default empty), summed in float32 and ORed voxel by voxel, then cut
    back into the leaves either side has, in OpenVDB leaf order."""
    allo = np.concatenate([np.asarray(a[0]).reshape(-1, 3), np.asarray(b[0]).reshape(-1, 3)]).astype(np.int64)
    lo = allo.min(0)
    ext = ((allo.max(0) - lo) // 8 + 1).astype(int)
    vals = [np.zeros((*(ext * 8), ncomp), dtype=np.float32) for _ in range(2)]
    bits = np.zeros(tuple(ext * 8), dtype=bool)
    have = np.zeros(tuple(ext), dtype=bool)
    for side, (o, m, v) in enumerate((a, b)):
        o = np.asarray(o).reshape(-1, 3).astype(np.int64)
        v = np.asarray(v, dtype=np.float32).reshape(len(o), 8, 8, 8, ncomp)
        mb = np.ones((len(o), 512), dtype=bool) if m is None else unpack(m)
        for i, oo in enumerate(o - lo):
            x, y, z = oo
            vals[side][x:x + 8, y:y + 8, z:z + 8] = v[i]
            bits[x:x + 8, y:y + 8, z:z + 8] |= mb[i].reshape(8, 8, 8)
            have[x // 8, y // 8, z // 8] = True
    total = vals[0] + vals[1]
    keep = np.argwhere(have)
    out_o = (keep * 8 + lo).astype(np.int32)
    out_v = np.stack([total[x * 8:x * 8 + 8, y * 8:y * 8 + 8, z * 8:z * 8 + 8].reshape(512, ncomp) for x, y, z in keep])
    out_m = pack(np.stack([bits[x * 8:x * 8 + 8, y * 8:y * 8 + 8, z * 8:z * 8 + 8].reshape(512) for x, y, z in keep]))
    order = fields.nanovdb_order(out_o)
    out_v = out_v[order].reshape(-1, ncomp)
    return out_o[order], out_m[order], out_v if ncomp == 3 else out_v.reshape(-1)


def side(seed, origins, ncomp, masked, neg_zero=True):
    rng = np.random.default_rng(seed)
    o = np.asarray(origins, dtype=np.int32)[rng.permutation(len(origins))]  # caller order, not OpenVDB order
    v = rng.standard_normal((len(o) * 512, ncomp)).astype(np.float32)
    if neg_zero:
        v[rng.random(v.shape) < 0.1] = -0.0
        v[rng.random(v.shape) < 0.05] = 0.0
    m = None
    if masked:
        bits = rng.random((len(o), 512)) < rng.choice([0.0, 0.01, 0.3, 1.0], size=(len(o), 1))
        m = pack(bits)
    return o, m, v if ncomp == 3 else v.reshape(-1)


def lattice(lo, hi):
    g = np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g * 8).astype(np.int32)


LAYOUTS = {
    "overlapping": (lattice(-2, 1), lattice(-1, 2)),
    "disjoint": (lattice(-2, 0), lattice(1, 3)),
    "identical": (lattice(-1, 2), lattice(-1, 2)),
    "one_empty": (lattice(0, 2), np.zeros((0, 3), dtype=np.int32)),
}


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.asarray(x, dtype=np.float32).view(np.uint32), np.asarray(y, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("masked", [(False, False), (True, False), (True, True)], ids=["nomasks", "amasks", "bothmasks"])
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_add_leaves_against_brute_force(layout, ncomp, masked):
    oa, ob = LAYOUTS[layout]
    seed = 11 * ncomp + len(oa) + 3 * masked[0] + masked[1]
    a = side(seed, oa, ncomp, masked[0])
    b = side(seed + 1, ob, ncomp, masked[1])
    got_o, got_m, got_v = leafio.add_leaves(a, b, ncomp)
    want_o, want_m, want_v = brute_force(a, b, ncomp)
    assert np.array_equal(got_o, want_o)
    assert np.array_equal(got_o, leafio.union_leaves(a[0], b[0])), "leaf order must be hns_union_leaves'"
    assert np.array_equal(got_m, want_m)
    assert same_bits(got_v, want_v)


def test_negative_zero_becomes_positive_where_one_side_lacks_the_leaf():
    o1 = np.array([[0, 0, 0]], dtype=np.int32)
    o2 = np.array([[8, 0, 0]], dtype=np.int32)
    nz = np.full(512, -0.0, dtype=np.float32)
    for a, b in (((o1, None, nz), (o2, None, nz)), ((o1, None, nz), (np.zeros((0, 3), np.int32), None, np.zeros(0, np.float32)))):
        _, m, v = leafio.add_leaves(a, b, 1)
        assert (v.view(np.uint32) == 0).all(), "-0.0f + (missing = +0.0f) must be +0.0f"
        assert (m == 0xFF).all()
    _, _, v = leafio.add_leaves((o1, None, nz), (o1, None, nz), 1)
    assert (v.view(np.uint32) == 0x80000000).all(), "-0.0f + -0.0f stays -0.0f"


def test_add_leaves_refusals():
    ok = (np.array([[0, 0, 0]], dtype=np.int32), None, np.zeros(512, dtype=np.float32))
    unaligned = (np.array([[4, 0, 0]], dtype=np.int32), None, np.zeros(512, dtype=np.float32))
    dup = (np.array([[8, 0, 0], [0, 8, 0], [8, 0, 0]], dtype=np.int32), None, np.zeros(3 * 512, dtype=np.float32))
    for a, b in ((unaligned, ok), (ok, unaligned), (dup, ok), (ok, dup)):
        with pytest.raises(_lib.HNSError) as e:
            leafio.add_leaves(a, b, 1)
        assert e.value.code == _lib.HNS_ERR_TOPOLOGY
    lib = _lib.load_library()
    n = _lib.C.c_uint64(0)
    o = ok[0]
    assert lib.hns_add_leaves(o.ctypes.data, 1, None, None, None, 0, None, None, 1, None, None, None, 0, _lib.C.byref(n)) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert lib.hns_add_leaves(o.ctypes.data, 1, None, ok[2].ctypes.data, None, 0, None, None, 2, None, None, None, 0, _lib.C.byref(n)) == _lib.HNS_ERR_INVALID_ARGUMENT
    # capacity: the query gives the count, a too-small output is refused
    assert lib.hns_add_leaves(o.ctypes.data, 1, None, ok[2].ctypes.data, dup[0].ctypes.data, 2, None, dup[2].ctypes.data, 1, None, None, None, 0,
                              _lib.C.byref(n)) == _lib.HNS_OK and n.value == 3
    out_v = np.zeros(3 * 512, dtype=np.float32)
    assert lib.hns_add_leaves(o.ctypes.data, 1, None, ok[2].ctypes.data, dup[0].ctypes.data, 2, None, dup[2].ctypes.data, 1, None, None, out_v.ctypes.data, 2,
                              _lib.C.byref(n)) == _lib.HNS_ERR_INVALID_ARGUMENT


def test_load_library_binds_the_source_symbols():
    lib = _lib.load_library()
    for name in ("hns_add_leaves", "hns_sim_regrid_sourced"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.hns_sim_regrid_sourced.restype is _lib.C.c_void_p
    assert [f[0] for f in _lib.hns_leaf_source._fields_] == ["name", "ncomp", "origins", "n_leaves", "masks", "values"]
