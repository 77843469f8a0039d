"""The device grid build's test cases, shared by the grid-build, origin-hash and pool-content tests: the launch-order rule and the origin hash restated in numpy, the
search for leaves that collide in a table, and the comparison of a device-built grid's tables with the host builder's."""
import numpy as np

from hnanosolver_amd import _lib, api, fields


def expected_sched(n):
    base, rem = n // 8, n % 8
    b = np.arange(n)
    x, i = b % 8, b // 8
    return (x * base + np.minimum(x, rem) + i).astype(np.int32)


def hash_origin(origins):
    """hns_originhash.hpp's hash_origin restated: (n, 3) 8-aligned origins -> uint32 (64-bit products, of which the low 32 bits are the 32-bit product)"""
    l = (np.asarray(origins, dtype=np.int64) >> 3).astype(np.uint64) & 0xFFFFFFFF
    h = (l[:, 0] * 0x9E3779B1) & 0xFFFFFFFF
    h ^= (l[:, 1] * 0x85EBCA77) & 0xFFFFFFFF
    h ^= (l[:, 2] * 0xC2B2AE3D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    return h.astype(np.uint32)


def home_slots(origins, slots):
    """the slot a probe for each origin starts at in a table of `slots` (a power of two) slots"""
    return (hash_origin(origins) & np.uint32(slots - 1)).astype(np.int64)


def box_leaves(lo=-6, hi=6):
    """the origins of the leaves with coordinates in [lo, hi)^3, x major"""
    r = np.arange(lo, hi)
    return (np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) * 8).astype(np.int32)


def assert_device_tables_match_host_builder(origins):
    """neighbour table, origin hash and launch order of a device-built grid against the host builder and the launch-order rule -> the device's three answers"""
    dev = api.create_grid_from_leaves(origins, 0.1)
    host = api.create_grid_from_leaves(origins, 0.1, _lib.HNS_GRID_HOST_ONLY)
    nbr_d, nbr_h = dev.neighbor_table(), host.neighbor_table()
    assert np.array_equal(nbr_d, nbr_h)
    # origin hash: same answers for voxels inside, next to and far from the domain
    rng = np.random.default_rng(7)
    c = fields.leaves_to_coords(origins)
    probes = np.concatenate([c[rng.integers(0, len(c), 4000)], c[rng.integers(0, len(c), 4000)] + rng.integers(-20, 21, (4000, 3)),
                             rng.integers(-2**31, 2**31 - 1, (2000, 3))]).astype(np.int64)
    probes = np.clip(probes, -2**31, 2**31 - 1).astype(np.int32)
    offsets = dev.offsets(probes)
    assert np.array_equal(offsets, host.offsets(probes))
    inside = dev.offsets(c[::97])
    assert np.array_equal(inside, np.arange(len(c), dtype=np.uint64)[::97] + 1)
    # launch order
    n = len(origins)
    sched = dev.launch_order()
    assert np.array_equal(np.sort(sched), np.arange(n))  # every leaf is worked on by exactly one workgroup
    assert np.array_equal(sched, expected_sched(n))
    dev.reset()
    host.reset()
    return {"neighbor_table": nbr_d, "offsets": offsets, "launch_order": sched}
