"""Point values added into fields, without a GPU: the host mirror hns_grid_splat_points (api.splat_points_host) against the numpy restatement of include/hns.h
(tests/splat_cases.py: restate) in every byte -- fields, status, rejected count, masks --, known answers, special values, wrap-around of the 64-bit accumulators and the
refusals. The device is held to this mirror in tests/test_splat_gpu.py. Nothing here has a tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import splat_cases as sp
from hnanosolver_amd import _lib, api, device

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_dev_splat_points", "hns_sim_splat_points", "hns_grid_splat_points")


def f32(*x):
    return np.array(x, dtype=F)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        header = f.read()
    decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S)
    assert decl, f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1
    assert lib.hns_version() == 100
    assert callable(device.splat_points) and callable(device.Sim.splat) and callable(api.splat_points_host)


def test_header_says_the_calls_are_not_mirrored_in_the_partitioned_sim():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        header = f.read()
    for name in ("hns_dev_splat_points", "hns_sim_splat_points"):
        comment = header[: header.index("int " + name)].rsplit("/*", 1)[1]
        assert "mirrored in hns_dist_*" in comment, name
    assert "cannot add leaves" in header[: header.index("int hns_sim_splat_points")].rsplit("/*", 1)[1].lower()


# ---------------------------------------------------------------------------------------------------------------
# 1. the mirror equals the restatement
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("q", sp.QUANTA)
@pytest.mark.parametrize("name", sp.GRIDS)
def test_mirror_equals_the_restatement(name, q):
    o, vel, phi, xyz, vals, vvals, masks = sp.case(name)
    G, g = sp.oracle_grid(name), sp.host_grid(o)
    fields, values = [phi[0], vel, phi[1]], [vals[0], vvals, vals[1]]
    for activate in (True, False):
        want, want_status, want_rej, want_masks, _ = sp.restate(G, fields, xyz, values, q, masks, activate)
        got, status, rej, got_masks = sp.mirror(g, fields, xyz, values, q, masks, activate)
        for i in range(len(fields)):
            assert sp.same_bytes(got[i], want[i]), f"{name} Q={q}: field {i} differs in {(got[i].view(np.uint32) != want[i].view(np.uint32)).sum()} words"
            assert not sp.same_bytes(got[i], fields[i]), "nothing was added"
        assert sp.same_bytes(status, want_status) and rej == want_rej == 0
        assert sp.same_bytes(got_masks, want_masks)
        assert sp.same_bytes(got_masks, masks) == (not activate)


@pytest.mark.parametrize("n", sp.COUNTS)
def test_mirror_equals_the_restatement_at_every_count(n):
    o, vel, phi, xyz, vals, vvals, _ = sp.case("ragged32")
    G, g = sp.oracle_grid("ragged32"), sp.host_grid(o)
    want, want_status, _, _, _ = sp.restate(G, [vel, phi[2]], xyz[:n], [vvals[:n], vals[2][:n]], -32)
    got, status, rej, _ = sp.mirror(g, [vel, phi[2]], xyz[:n], [vvals[:n], vals[2][:n]], -32)
    assert sp.same_bytes(got[0], want[0]) and sp.same_bytes(got[1], want[1]) and sp.same_bytes(status, want_status) and rej == 0


def test_output_i_of_a_shared_call_equals_a_call_with_field_i_alone():
    o, vel, phi, xyz, vals, vvals, _ = sp.case("sparse_far")
    g = sp.host_grid(o)
    fields, values = sp.channel_sets("sparse_far")["5float+vec3"]
    together = sp.mirror(g, fields, xyz, values)[0]
    for i in range(len(fields)):
        assert sp.same_bytes(sp.mirror(g, [fields[i]], xyz, [values[i]])[0][0], together[i]), i


# ---------------------------------------------------------------------------------------------------------------
# 2. known answers
# ---------------------------------------------------------------------------------------------------------------

ONE = np.array([[8, -16, 24]], dtype=np.int32)  # special_cases.LEAF_SETS["one_leaf"]


def local(i, j, k):
    return (i << 6) | (j << 3) | k


def test_a_point_on_a_voxel_adds_its_rounded_value_there_and_nothing_else():
    g = sp.host_grid(ONE)
    v = F(0.1)  # not a multiple of 2^-32
    field = np.full(512, F(-0.0))
    field[local(3, 4, 5)] = F(2.0)
    got, status, rej, _ = sp.mirror(g, [field], f32([11.0, -12.0, 29.0]), [f32(v)])
    want = field.copy()
    want[local(3, 4, 5)] = F(2.0) + F(np.rint(np.float64(v) * 2.0 ** 32) * 2.0 ** -32)
    assert sp.same_bytes(got[0], want) and status.tolist() == [8] and rej == 0
    assert np.signbit(got[0][np.arange(512) != local(3, 4, 5)]).all()  # every -0.0f kept its sign: a zero term adds nothing


def test_a_point_at_the_centre_of_a_cell_adds_an_eighth_to_eight_voxels():
    g = sp.host_grid(ONE)
    got, status, rej, _ = sp.mirror(g, [np.zeros(512, F)], f32([9.5, -14.5, 26.5]), [f32(1.0)])
    want = np.zeros(512, F)
    for c in range(8):
        want[local(1 + (c >> 2), 1 + ((c >> 1) & 1), 2 + (c & 1))] = 0.125
    assert sp.same_bytes(got[0], want) and status.tolist() == [8] and rej == 0


def test_the_totals_of_the_accumulators_equal_the_total_of_the_accepted_terms():
    """positions on quarter voxels and values on multiples of 2^-10: every weight, term and sum is exact at Q = -32, so a zero field ends as accumulator * 2^Q exactly"""
    o = sp.case("ragged32")[0]
    G, g = sp.oracle_grid("ragged32"), sp.host_grid(o)
    rng = np.random.default_rng(9)
    xyz = (o[rng.integers(0, len(o), 600)] + rng.integers(0, 40, (600, 3)) / 4.0 - 1.0).astype(F)
    vals = (rng.integers(-4096, 4096, 600) / 1024.0).astype(F)
    zero = np.zeros(G.N, F)
    _, _, rej, _, ks = sp.restate(G, [zero], xyz, [vals], -32)
    got = sp.mirror(g, [zero], xyz, [vals])[0][0]
    total = int(np.rint(got.astype(np.float64) * 2.0 ** 32).astype(np.int64).sum())
    assert rej == 0 and len(ks[0]) > 1000 and total == int(ks[0].sum()) and total != 0


# ---------------------------------------------------------------------------------------------------------------
# 3. special values, wrap-around
# ---------------------------------------------------------------------------------------------------------------


def test_positions_that_are_not_finite_or_far_beyond_the_range_land_nowhere():
    o = sp.case("ragged32")[0]  # holds the leaf of the origin: a NaN position's cell, were it looked up, would land
    G, g = sp.oracle_grid("ragged32"), sp.host_grid(o)
    xyz = f32([np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [3e9, 1, 1], [1, -3e9, 1], [3e9, 3e9, 3e9], [1.5, 1.5, 1.5])
    field = np.zeros(G.N, F)
    got, status, rej, _ = sp.mirror(g, [field], xyz, [np.ones(len(xyz), F)])
    want, want_status, want_rej, _, _ = sp.restate(G, [field], xyz, [np.ones(len(xyz), F)], -32)
    assert status.tolist() == [0, 0, 0, 0, 0, 0, 8] == want_status.tolist() and rej == want_rej == 0
    assert sp.same_bytes(got[0], want[0]) and got[0].sum() == 1.0


def test_values_that_are_not_finite_or_beyond_the_bound_are_counted_and_add_nothing():
    g, G = sp.host_grid(ONE), sp.OracleGrid(ONE)
    xyz = f32([9.5, -14.5, 26.5], [9.5, -14.5, 26.5], [9.5, -14.5, 26.5], [9.5, -14.5, 26.5], [10.0, -14.0, 27.0], [9.25, -14.5, 26.5])
    vals = f32(np.nan, np.inf, -np.inf, 2.0 ** 34, np.inf, 2.0 ** 32)  # 2^34 / 8 = 2^31 quanta of 2^-32 = 2^63: beyond; inf * 0 = NaN on seven taps of the fifth point
    field = np.full(512, F(-0.0))
    got, status, rej, _ = sp.mirror(g, [field], xyz, [vals], -32)
    want, _, want_rej, _, _ = sp.restate(G, [field], xyz, [vals], -32)
    # the last point: weights 3/16 and 1/16 of 2^32 -> 3 * 2^60 and 2^60 quanta: accepted
    assert rej == want_rej == 5 * 8 and (status == 8).all()
    assert sp.same_bytes(got[0], want[0]) and (got[0] != 0).sum() == 8 and np.signbit(got[0][got[0] == 0]).all()


@pytest.mark.parametrize("q", (0, -8, -40))
@pytest.mark.parametrize("m", (2, 4, 5, 8))
def test_accumulators_wrap_modulo_two_to_the_64(m, q):
    """m terms of 2^61 quanta into one voxel: 4 of them are -2^63 as an int64, 8 of them are 0 and leave the voxel's bytes"""
    g, G = sp.host_grid(ONE), sp.OracleGrid(ONE)
    xyz = np.tile(f32([10.0, -14.0, 27.0]), (m, 1))
    vals = np.full(m, F(2.0 ** (61 + q)))
    field = np.full(512, F(-0.0))
    got, _, rej, _ = sp.mirror(g, [field], xyz, [vals], q)
    want, _, want_rej, _, _ = sp.restate(G, [field], xyz, [vals], q)
    assert rej == want_rej == 0 and sp.same_bytes(got[0], want[0])
    total = (m * 2 ** 61 + 2 ** 63) % 2 ** 64 - 2 ** 63
    v = got[0][local(2, 2, 3)]
    assert v == F(np.float64(total) * 2.0 ** q) and (np.signbit(v) if total == 0 else v != 0)


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------


def test_every_refusal_leaves_all_outputs_untouched_with_its_code_and_message():
    lib = _lib.load_library()
    g = sp.host_grid(ONE)
    n = 5
    a, b = np.full(512, F(7.0)), np.full((512, 3), F(7.0))
    xyz, va, vb = np.tile(f32(9.5, -14.5, 26.5), (n, 1)), np.ones(n, F), np.ones((n, 3), F)
    status, masks, rejected = np.full(n, 9, np.uint8), np.full(64, 3, np.uint8), C.c_uint64(5)
    P = lambda *arrays: (C.c_void_p * max(1, len(arrays)))(*[None if x is None else x.ctypes.data for x in arrays])
    NC = lambda *c: (C.c_int * max(1, len(c)))(*c)
    rej, other = C.byref(rejected), np.zeros(1, np.uint64)
    ok = dict(g=g.ptr, fields=P(a, b), ncomp=NC(1, 3), k=2, xyz=xyz.ctypes.data, values=P(va, vb), n=n, q=-32, masks=masks.ctypes.data, act=1,
              status=status.ctypes.data, rej=rej)
    bad = [
        (dict(g=None), "null grid"),
        (dict(fields=None), "null list"), (dict(ncomp=None), "null list"), (dict(values=None), "null list"),
        (dict(fields=P(a, None)), "fields[1] is null"), (dict(values=P(None, vb)), "values[0] is null"), (dict(xyz=None), "xyz is null"),
        (dict(ncomp=NC(1, 2)), "ncomp[1] is 2"), (dict(k=0), "n_fields is 0"), (dict(k=9), "n_fields is 9"),
        (dict(n=2 ** 31), "n is above 2^31 - 1"), (dict(q=-41), "log2_quantum is -41"), (dict(q=1), "log2_quantum is 1"),
        (dict(fields=P(a, a), ncomp=NC(1, 1), values=P(va, va)), "fields[1] is fields[0]"),
        (dict(fields=P(b, xyz), ncomp=NC(3, 3)), "fields[1] is xyz"),
        (dict(values=P(va, a)), "fields[0] is values[1]"),
        (dict(fields=P(status, b)), "fields[0] is status"),
        (dict(fields=P(a, other), rej=C.cast(other.ctypes.data, C.POINTER(C.c_uint64))), "fields[1] is d_rejected"),
    ]
    for change, text in bad:
        kw = dict(ok, **change)
        rc = lib.hns_grid_splat_points(kw["g"], kw["fields"], kw["ncomp"], kw["k"], kw["xyz"], kw["values"], kw["n"], kw["q"], kw["masks"], kw["act"], kw["status"],
                                       kw["rej"])
        msg = lib.hns_last_error().decode()
        assert rc == _lib.HNS_ERR_INVALID_ARGUMENT, (text, rc, msg)
        assert "hns_grid_splat_points" in msg and text in msg, (text, msg)
        assert (a == 7).all() and (b == 7).all() and (status == 9).all() and (masks == 3).all() and rejected.value == 5 and (xyz == f32(9.5, -14.5, 26.5)).all(), text
    # and the call they all vary is accepted
    assert lib.hns_grid_splat_points(ok["g"], ok["fields"], ok["ncomp"], 2, ok["xyz"], ok["values"], n, -32, ok["masks"], 1, ok["status"], rej) == 0
    assert (status == 8).all() and rejected.value == 5 and not (a == 7).all() and not (b == 7).all() and not (masks == 3).all()


def test_no_points_look_at_no_pointer_and_the_device_calls_fail_loudly_without_a_device():
    lib = _lib.load_library()
    g = sp.host_grid(ONE)
    P = (C.c_void_p * 1)(None)
    assert lib.hns_grid_splat_points(g.ptr, P, (C.c_int * 1)(1), 1, None, P, 0, -32, None, 1, None, None) == 0
    if lib.hns_device_count() > 0:
        return
    a, xyz, va = np.full(512, F(7.0)), np.full((3, 3), F(9.5)), np.ones(3, F)
    F1, V1 = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(va.ctypes.data)
    assert lib.hns_dev_splat_points(g.ptr, F1, (C.c_int * 1)(1), 1, xyz.ctypes.data, V1, 3, -32, None, None, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_dev_splat_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    names = (C.c_char_p * 1)(b"density")
    assert lib.hns_sim_splat_points(None, names, 1, None, xyz.ctypes.data, V1, 3, -32, 1, None, None, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_sim_splat_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    assert (a == 7).all()
