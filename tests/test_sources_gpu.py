"""hns_sim_regrid_sourced on the MI355X: the sourced device regrid against the host chain it stands for (hns_sim_download -> hns_add_leaves per
source -> hns_dilate_leaf_masks of the summed velocity -> union with the SDF's leaves -> hns_gather_leaves -> new grid -> hns_sim_upload), bit for
bit: leaves and their order, masks, every field and fill, and the substeps that follow; and every refusal."""
import ctypes as C

import numpy as np
import pytest

from frame_cases import (COMBUST, assert_same, download, emitter, host_chain, make_sim, make_sources, random_leaves, random_masks, random_state,
                         sdf_source)
from hnanosolver_amd import _lib, api, fields

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("where", ["inside", "outside", "straddling"])
@pytest.mark.parametrize("kind", ["velocity", "float", "mixed"])
@pytest.mark.parametrize("with_sdf", [False, True], ids=["nosdf", "sdf"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_sourced_regrid_matches_the_host_chain(p, with_sdf, kind, where):
    names = COMBUST + (["collision_sdf"] if with_sdf else [])
    seed = 13 * p + 5 * with_sdf + len(kind) + len(where)
    o = random_leaves(seed)
    m = random_masks(seed + 1, len(o))
    st = random_state(seed + 2, len(o), names)
    g, s = make_sim(o, names, st, m)
    sdf = sdf_source(seed + 3, o) if with_sdf else None
    src = make_sources(seed + 4, o, kind, where)
    ng = s.regrid(p, sdf, src)
    dom, dm, want = host_chain(o, m, st, names, p, src, sdf)
    assert s.grid is ng and ng.ptr != g.ptr and g.leaf_count() == len(o)
    assert np.array_equal(ng.coords()[::512], dom), "leaf set / OpenVDB order"
    assert np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"p={p} {kind} {where}")
    assert all(v >= 0 for v in s.regrid_times().values())
    s.close()


def test_float_source_outside_the_final_domain_is_dropped():
    names = COMBUST
    o = random_leaves(21)
    st = random_state(22, len(o), names)
    g, s = make_sim(o, names, st)
    rng = np.random.default_rng(23)
    far = (np.array([[100, 0, 0], [100, 1, 0], [101, 0, -3]], dtype=np.int32) * 8)
    src = {"fuel": (far, None, rng.standard_normal(len(far) * 512).astype(np.float32)),
           "density": (np.concatenate([o[:3], far[:1]]), None, rng.standard_normal(4 * 512).astype(np.float32))}
    ng = s.regrid(1, None, src)
    dom, dm, want = host_chain(o, None, st, names, 1, src)
    got = ng.coords()[::512]
    assert np.array_equal(got, dom)
    assert not any((got == f).all(1).any() for f in far), "a float source leaf outside the domain must not join it"
    assert_same(download(s, names), want, "dropped source")
    s.close()


@pytest.mark.parametrize("with_sdf", [False, True], ids=["nosdf", "sdf"])
def test_zero_sources_is_hns_sim_regrid(with_sdf):
    names = COMBUST + (["collision_sdf"] if with_sdf else [])
    o = random_leaves(31)
    m = random_masks(32, len(o))
    st = random_state(33, len(o), names)
    sdf = sdf_source(34, o) if with_sdf else None
    g1, s1 = make_sim(o, names, st, m)
    g2, s2 = make_sim(o, names, st, m)
    a = s1.regrid(2, sdf)
    b = s2.regrid(2, sdf, {})
    assert np.array_equal(a.coords(), b.coords())
    assert np.array_equal(s1.active_masks(), s2.active_masks())
    assert_same(download(s1, names), download(s2, names), "zero sources")  # -0.0 kept: no sum on unsourced fields
    s1.close(), s2.close()


def test_two_runs_give_the_same_bytes():
    names = COMBUST + ["collision_sdf"]
    o = random_leaves(41)
    m = random_masks(42, len(o))
    st = random_state(43, len(o), names)
    sdf = sdf_source(44, o)
    src = make_sources(45, o, "mixed", "straddling")
    res = []
    for _ in range(2):
        g, s = make_sim(o, names, st, m)
        ng = s.regrid(9, sdf, src)
        res.append((ng.coords(), s.active_masks(), download(s, names)))
        s.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert_same(res[0][2], res[1][2], "second run")


def test_four_frame_chain_against_the_host_chain():
    R = 32
    names = COMBUST
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + names}
    g, s = make_sim(o, names, st, None, 1.0 / R)  # a new sim: all voxels active
    grids = [g]
    ho, hm, hst = o, None, st
    params = api.CombustionParams()
    for frame in range(4):
        src = emitter(R, frame)
        grids.append(s.regrid(1, None, src))
        ho, hm, hst = host_chain(ho, hm, hst, names, 1, src)
        hg, hs = make_sim(ho, names, hst, None, 1.0 / R)
        assert np.array_equal(s.grid.coords()[::512], ho) and np.array_equal(s.active_masks(), hm)
        assert_same(download(s, names), hst, f"frame {frame} regrid")
        for _ in range(2):
            s.substep(4, 1.0 / 24, 1.0 / R, params, False)
            hs.substep(4, 1.0 / 24, 1.0 / R, params, False)
        got, hst = download(s, names), download(hs, names)
        assert_same(got, hst, f"frame {frame}")
        hs.close()
    assert len(ho) > len(o)
    s.close()


def raw_regrid(sim, p, entries):
    """hns_sim_regrid_sourced with hand-built hns_leaf_source entries (name, ncomp, origins, masks, values, n_leaves) -> (grid ptr, err, message)"""
    lib = _lib.load_library()
    arr = (_lib.hns_leaf_source * max(1, len(entries)))()
    keep = []
    for i, (name, nc, o, m, v, n) in enumerate(entries):
        b = None if name is None else name.encode()
        keep += [b, o, m, v]
        arr[i].name, arr[i].ncomp, arr[i].n_leaves = b, nc, n
        arr[i].origins = None if o is None else o.ctypes.data
        arr[i].masks = None if m is None else m.ctypes.data
        arr[i].values = None if v is None else v.ctypes.data
    err = C.c_int(0)
    ptr = lib.hns_sim_regrid_sourced(sim._ptr, p, arr, len(entries), None, 0, None, None, None, C.byref(err))
    return ptr, err.value, lib.hns_last_error().decode()


def test_refusals_leave_the_sim_as_it_was():
    names = COMBUST + ["collision_sdf"]
    o = random_leaves(51)
    st = random_state(52, len(o), names)
    m = random_masks(53, len(o))
    g, s = make_sim(o, names, st, m)

    def unchanged():
        assert s.grid is g and np.array_equal(g.coords()[::512], o)
        assert np.array_equal(s.active_masks(), m)
        assert_same(download(s, names), st, "after a refusal")

    one = np.array([[0, 0, 0]], dtype=np.int32)
    v1 = np.ones(512, dtype=np.float32)
    v3 = np.ones((512, 3), dtype=np.float32)
    far = np.array([[800, 0, 0], [808, 0, 0], [800, 0, 0]], dtype=np.int32)  # duplicated, and wholly outside the domain
    cases = [
        ([("smoke", 1, one, None, v1, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "no float field 'smoke'"),
        ([("collision_sdf", 1, one, None, v1, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "'collision_sdf' cannot be a source"),
        ([("vel", 3, one, None, v3, 1), ("v2", 3, one, None, v3, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "second velocity source"),
        ([("fuel", 1, one, None, v1, 1), ("fuel", 1, one, None, v1, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "second source for 'fuel'"),
        ([("fuel", 2, one, None, v1, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "ncomp 2"),
        ([("density", 3, one, None, v3, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "ncomp 3 under the float field name 'density'"),
        ([("fuel", 1, one, None, None, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "values NULL"),
        ([("vel", 3, one, None, None, 1)], _lib.HNS_ERR_INVALID_ARGUMENT, "values NULL"),
        ([("fuel", 1, np.array([[4, 0, 0]], dtype=np.int32), None, v1, 1)], _lib.HNS_ERR_TOPOLOGY, "not 8-aligned"),
        ([("vel", 3, np.array([[0, 0, 12]], dtype=np.int32), None, v3, 1)], _lib.HNS_ERR_TOPOLOGY, "not 8-aligned"),
        ([("fuel", 1, far, None, np.ones(3 * 512, dtype=np.float32), 3)], _lib.HNS_ERR_TOPOLOGY, "duplicate leaf origin"),
        ([("vel", 3, far, None, np.ones((3 * 512, 3), dtype=np.float32), 3)], _lib.HNS_ERR_TOPOLOGY, "duplicate leaf origin"),
        ([("density", 1, one, None, v1, 1), ("vel", 3, far, None, np.ones((3 * 512, 3), dtype=np.float32), 3)], _lib.HNS_ERR_TOPOLOGY, "source 1 ('vel')"),
    ]
    for entries, code, msg in cases:
        ptr, err, text = raw_regrid(s, 1, entries)
        assert not ptr and err == code, (entries[0][:2], err, text)
        assert msg in text and text.startswith("hns_sim_regrid_sourced:"), text
        unchanged()
    with pytest.raises(ValueError, match="no float field"):  # the Python wrapper passes the refusal on
        s.regrid(1, None, {"smoke": (one, None, v1)})
    unchanged()
    # still usable: a good sourced regrid afterwards matches the host chain
    src = {"fuel": (one, None, v1), "vel": (one, None, v3)}
    s.regrid(1, None, src)
    dom, dm, want = host_chain(o, m, st, names, 1, src)
    assert np.array_equal(s.grid.coords()[::512], dom)
    assert_same(download(s, names), want, "after the refusals")
    s.close()
