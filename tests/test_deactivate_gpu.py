"""hns_sim_deactivate on the MI355X: device masks and counts against the host mirror (hns_deactivate_leaf_masks) byte for byte, fields untouched;
the regrid after it against the host chain (download -> hns_deactivate_leaf_masks -> hns_add_leaves per source -> hns_dilate_leaf_masks -> union
with the SDF -> hns_gather_leaves) bit for bit; a quiet cluster of leaves dropped; a six-frame chain; the empty domain; refusals and determinism."""
import ctypes as C

import numpy as np
import pytest

from hnanosolver_amd import _lib, api, fields
from frame_cases import (COMBUST, assert_same, download, emitter, frame_chain, host_chain, host_deactivate, make_sim, make_sources, random_leaves,
                         random_masks, sdf_source)

pytestmark = pytest.mark.gpu


def planted(rng, shape, tol):
    """standard normal values with long quiet (+-0) stretches and planted NaN, +-inf, +-tol and the next float above tol"""
    v = (rng.standard_normal(shape) * (2.0 * tol if tol > 0 else 1.0)).astype(np.float32)
    flat = v.reshape(-1)
    t = np.float32(tol)
    above = np.nextafter(t, np.float32(np.inf))
    for sv in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), t, -t, above, -above, np.float32(-0.0)):
        flat[rng.random(flat.size) < 0.01] = sv
    quiet = rng.random(flat.size) < 0.4
    flat[quiet] = np.where(rng.random(quiet.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    return v


def quiet_state(seed, n, names, tol, quiet_leaves=()):
    """fields of n leaves: planted values, and every value of the leaves in quiet_leaves +-0 (or exactly tol)"""
    rng = np.random.default_rng(seed)
    st = {"vel": planted(rng, (n * 512, 3), tol)}
    for k in names:
        st[k] = planted(rng, (n * 512,), tol)
    for k in st:
        v = st[k].reshape(n, -1)
        for i in quiet_leaves:
            v[i] = np.where(rng.random(v.shape[1]) < 0.5, np.float32(-0.0), np.float32(tol))
    return st


CASES = {
    "velocity0": ({}, 0.0),
    "floats": ({"density": 0.25, "fuel": 0.0}, None),
    "mixed": ({"density": 0.25, "temperature": 1.0}, 0.25),
    "inf": ({"density": float("inf")}, float("inf")),
}


@pytest.mark.parametrize("masked", [False, True], ids=["allactive", "masks"])
@pytest.mark.parametrize("case", list(CASES))
def test_device_masks_match_the_host_mirror(case, masked):
    names = COMBUST + ["collision_sdf"]
    tolerances, vtol = CASES[case]
    seed = len(case) * 3 + masked
    o = random_leaves(seed, n=60)
    st = quiet_state(seed + 1, len(o), names, 0.25, quiet_leaves=(0, 3))
    m = random_masks(seed + 2, len(o)) if masked else None
    g, s = make_sim(o, names, st, m)
    want, want_counts = host_deactivate(m, st, tolerances, vtol)
    counts = s.deactivate(tolerances, vtol, counts=True)
    assert np.array_equal(s.active_masks(), want), case
    assert counts == want_counts
    assert_same(download(s, names), st, "fields after deactivate")
    # asynchronous form on a second sim: the same bytes
    g2, s2 = make_sim(o, names, st, m)
    assert s2.deactivate(tolerances, vtol) is None
    assert np.array_equal(s2.active_masks(), want)
    # a second call only clears (here: nothing more, same fields)
    assert s.deactivate(tolerances, vtol, counts=True) == want_counts
    assert np.array_equal(s.active_masks(), want)
    s.close(), s2.close()


@pytest.mark.parametrize("sourced", [False, True], ids=["plain", "sourced"])
@pytest.mark.parametrize("with_sdf", [False, True], ids=["nosdf", "sdf"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_regrid_after_deactivation_matches_the_host_chain(p, with_sdf, sourced):
    names = COMBUST + (["collision_sdf"] if with_sdf else [])
    seed = 17 * p + 3 * with_sdf + sourced
    o = random_leaves(seed, n=40)
    st = quiet_state(seed + 1, len(o), names, 0.5, quiet_leaves=range(0, len(o), 3))
    m = random_masks(seed + 2, len(o))
    g, s = make_sim(o, names, st, m)
    sdf = sdf_source(seed + 3, o) if with_sdf else None
    src = make_sources(seed + 4, o, "mixed", "straddling") if sourced else {}
    tolerances, vtol = {"density": 0.5, "temperature": 0.5}, 0.5
    s.deactivate(tolerances, vtol)
    ng = s.regrid(p, sdf, src) if sourced else s.regrid(p, sdf)
    hm, _ = host_deactivate(m, st, tolerances, vtol)
    dom, dm, want = host_chain(o, hm, st, names, p, src, sdf)
    assert np.array_equal(ng.coords()[::512], dom), "leaf set / OpenVDB order"
    assert np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"p={p}")
    s.close()


def test_a_quiet_cluster_is_dropped():
    names = COMBUST
    lat = np.stack(np.meshgrid(*[np.arange(0, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    near, far = lat * 8, (lat + 20) * 8  # two 3^3 blocks of leaves, far apart
    o = np.concatenate([near, far]).astype(np.int32)
    centre = 13  # leaf (8, 8, 8) of the near block: the only one with anything going on
    rng = np.random.default_rng(3)
    st = {"vel": rng.standard_normal((len(o) * 512, 3)).astype(np.float32)}
    for k in names:
        st[k] = rng.standard_normal(len(o) * 512).astype(np.float32)
    for k in st:
        v = st[k].reshape(len(o), -1)
        v[np.arange(len(o)) != centre] = 0.0
    g, s = make_sim(o, names, st)
    assert s.deactivate({"density": 0.0}, 0.0, counts=True) == (512, 1)
    ng = s.regrid(1)
    got = ng.coords()[::512]
    assert not any((got == f).all(1).any() for f in far), "the quiet block must go"
    assert len(got) == len(near) < len(o), "the centre leaf dilated by one voxel: the near block, nothing else"
    hm, _ = host_deactivate(None, st, {"density": 0.0}, 0.0)
    dom, dm, want = host_chain(o, hm, st, names, 1, {})
    assert np.array_equal(got, dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "after the drop")
    s.close()


def chain_state(R):
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    blob = st["density"].copy()
    st["vel"] *= blob[:, None]  # motion only where the smoke is: the far corners are quiet
    return o, {k: st[k] for k in ["vel"] + COMBUST}


def test_six_frame_chain_against_the_host_chain():
    R = 32
    names = COMBUST
    o, st = chain_state(R)
    params = api.CombustionParams()
    g, s = make_sim(o, names, st, None, 1.0 / R)
    g0, s0 = make_sim(o, names, st, None, 1.0 / R)  # the same chain without deactivation
    frame_chain(s, names, (o, None, st), 6, lambda frame, origins: (1, None, emitter(R, frame)), lambda sim, frame: sim.substep(4, 1.0 / 24, 1.0 / R, params, False),
                {"density": 1e-2}, 0.1, 1.0 / R, shadows=(s0,), keep=[g, g0])
    assert s.grid.leaf_count() < s0.grid.leaf_count(), (s.grid.leaf_count(), s0.grid.leaf_count())
    s.close(), s0.close()


def test_empty_domain_refuses_then_a_sourced_regrid_works():
    names = COMBUST
    o = random_leaves(61)
    st = {"vel": np.zeros((len(o) * 512, 3), np.float32)}
    for k in names:
        st[k] = np.full(len(o) * 512, -0.0, np.float32)
    g, s = make_sim(o, names, st)
    assert s.deactivate({"density": 0.0}, 0.0, counts=True) == (0, 0)
    zero = np.zeros((len(o), 64), np.uint8)
    with pytest.raises(_lib.HNSError, match="No active voxels") as e:
        s.regrid(1)
    assert e.value.code == _lib.HNS_ERR_RUNTIME
    assert s.grid is g and np.array_equal(s.active_masks(), zero)
    assert_same(download(s, names), st, "after the refused regrid")
    src = make_sources(62, o, "mixed", "straddling")
    ng = s.regrid(1, None, src)
    dom, dm, want = host_chain(o, zero, st, names, 1, src)
    assert np.array_equal(ng.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "sourced regrid from an empty domain")
    s.close()


def raw_deactivate(sim, entries, counts=False):
    """hns_sim_deactivate with hand-built entries (name, ncomp, tolerance) -> (code, message)"""
    lib = _lib.load_library()
    arr = (_lib.hns_activity_field * max(1, len(entries)))()
    for i, (name, nc, tol) in enumerate(entries):
        arr[i].name, arr[i].ncomp, arr[i].tolerance = None if name is None else name.encode(), nc, tol
    out = (C.c_uint64 * 2)()
    rc = lib.hns_sim_deactivate(sim._ptr, arr, len(entries), out if counts else None, None)
    return rc, lib.hns_last_error().decode()


@pytest.mark.parametrize("masked", [False, True], ids=["allactive", "masks"])
def test_refusals_leave_the_masks_and_two_runs_agree(masked):
    names = COMBUST + ["collision_sdf"]
    o = random_leaves(71)
    st = quiet_state(72, len(o), names, 0.5)
    m = random_masks(73, len(o)) if masked else None
    g, s = make_sim(o, names, st, m)
    before = s.active_masks()
    cases = [
        ([], "bad field list"),
        ([("smoke", 1, 0.0)], "the sim has no float field 'smoke'"),
        ([("collision_sdf", 1, 0.0)], "'collision_sdf' cannot be deactivated"),
        ([("density", 1, 0.0), ("density", 1, 1.0)], "a second entry for 'density'"),
        ([("vel", 3, 0.0), (None, 3, 0.0)], "a second velocity entry"),
        ([("fuel", 2, 0.0)], "ncomp 2"),
        ([("density", 3, 0.0)], "ncomp 3 under the float field name 'density'"),
        ([("density", 1, -0.5)], "tolerance -0.5"),
        ([("fuel", 1, 0.0), (None, 3, float("nan"))], "tolerance nan"),
    ]
    for entries, msg in cases:
        for counts in (False, True):
            rc, text = raw_deactivate(s, entries, counts)
            assert rc == _lib.HNS_ERR_INVALID_ARGUMENT, (entries, rc, text)
            assert text.startswith("hns_sim_deactivate:") and msg in text, text
            assert np.array_equal(s.active_masks(), before)
    lib = _lib.load_library()
    assert lib.hns_sim_deactivate(s._ptr, None, 1, None, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="no float field 'smoke'"):
        s.deactivate({"smoke": 0.0})
    assert np.array_equal(s.active_masks(), before)
    assert_same(download(s, names), st, "after the refusals")
    # still usable, and deterministic: two sims, the same bytes
    res = []
    for sim in (s, make_sim(o, names, st, m)[1]):
        c = sim.deactivate({"density": 0.5, "waste": 0.5}, 0.5, counts=True)
        ng = sim.regrid(2)
        res.append((c, ng.coords(), sim.active_masks(), download(sim, names)))
        sim.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert_same(res[0][3], res[1][3], "second run")
