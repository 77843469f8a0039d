"""hns_sim_regrid on the MI355X: the device regrid against the host chain it replaces (hns_sim_download -> hns_dilate_leaf_masks -> union with the
SDF's leaves -> hns_gather_leaves -> new grid -> hns_sim_upload), bit for bit: leaves and their order, masks, every field and fill, and the substeps
that follow."""
import numpy as np
import pytest

from frame_cases import COMBUST, assert_same, download, host_chain, make_sim, pack, random_leaves, random_masks, random_state, sdf_source
from hnanosolver_amd import _lib, api, fields

pytestmark = pytest.mark.gpu


CASES = [("s1", ["density"], False), ("s5", COMBUST, False), ("s5sdf", COMBUST + ["collision_sdf"], False), ("s5sdf_src", COMBUST + ["collision_sdf"], True)]


@pytest.mark.parametrize("p", [0, 1, 2, 8, 9, 17])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_regrid_matches_the_host_chain(case, p):
    _, names, with_src = case
    seed = 7 * p + len(names) + with_src
    o = random_leaves(seed)
    m = random_masks(seed + 1, len(o))
    st = random_state(seed + 2, len(o), names)
    g, s = make_sim(o, names, st, m)
    sdf = sdf_source(seed + 3, o) if with_src else None
    ng = s.regrid(p, sdf)
    dom, dm, want = host_chain(o, m, st, names, p, sdf=sdf)
    assert s.grid is ng and ng.ptr != g.ptr and g.leaf_count() == len(o)
    assert np.array_equal(ng.coords()[::512], dom), "leaf set / OpenVDB order"
    assert np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"p={p}")
    # determinism: a second run from the same state gives the same bytes
    g2, s2 = make_sim(o, names, st, m)
    s2.regrid(p, sdf)
    assert_same(download(s2, names), want, "second run")
    assert np.array_equal(s2.active_masks(), dm)
    t = s.regrid_times()
    assert all(v >= 0 for v in t.values())
    s.close(), s2.close()


@pytest.mark.parametrize("collision", [False, True])
def test_substeps_after_regrid_match_a_fresh_sim(collision):
    R = 32
    o = fields.dense_leaves(R)[::-1].copy()  # caller order reversed: the regrid's OpenVDB order moves element 0
    o = o[np.random.default_rng(1).permutation(len(o))]
    names = COMBUST + ["collision_sdf"]
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + COMBUST}
    st["collision_sdf"] = np.full(len(o) * 512, 5.0, dtype=np.float32)
    bits = np.zeros((len(o), 512), dtype=bool)
    bits[:, :448] = True  # x < 7 active: the dilation by 1 completes some leaves and reaches the next ring
    m = pack(bits)
    g, s = make_sim(o, names, st, m, 1.0 / R)
    for _ in range(2):  # stale scratch in the old arena
        s.substep(5, 1.0 / 24, 1.0 / R, api.CombustionParams(), collision)
    st1 = download(s, names)
    s.regrid(1)
    dom, dm, want = host_chain(o, m, st1, names, 1)
    g2, s2 = make_sim(dom, names, want, None, 1.0 / R)
    assert_same(download(s, names), want, "regrid")
    for _ in range(3):
        s.substep(5, 1.0 / 24, 1.0 / R, api.CombustionParams(), collision)
        s2.substep(5, 1.0 / 24, 1.0 / R, api.CombustionParams(), collision)
    assert_same(download(s, names), download(s2, names), "after substeps")
    s.close(), s2.close()


@pytest.mark.parametrize("p", [1, 8])
def test_four_frame_chain_against_the_host_chain(p):
    R = 32
    names = COMBUST
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + names}
    m = np.full((len(o), 64), 0xFF, dtype=np.uint8)
    g, s = make_sim(o, names, st, None, 1.0 / R)  # a new sim: all voxels active
    grids = [g]
    ho, hm, hst = o, m, st
    counts = []
    params = api.CombustionParams()
    for frame in range(4):
        grids.append(s.regrid(p))
        ho, hm, hst = host_chain(ho, hm, hst, names, p)
        hg, hs = make_sim(ho, names, hst, None, 1.0 / R)
        assert np.array_equal(s.grid.coords()[::512], ho) and np.array_equal(s.active_masks(), hm)
        for _ in range(2):
            s.substep(4, 1.0 / 24, 1.0 / R, params, False)
            hs.substep(4, 1.0 / 24, 1.0 / R, params, False)
        got, hst = download(s, names), download(hs, names)
        assert_same(got, hst, f"frame {frame}")
        counts.append(len(ho))
        hs.close()
    assert counts == ([216] * 4 if p == 1 else [216, 512, 1000, 1728])
    s.close()


def test_identity_regrid():
    o = fields.plume_leaves(8, 1.0, 0.3)  # OpenVDB order already
    names = ["density", "collision_sdf"]
    st = random_state(3, len(o), names)
    g, s = make_sim(o, names, st)
    ng = s.regrid(0)
    assert np.array_equal(ng.coords(), g.coords())
    assert_same(download(s, names), st, "identity")
    assert (s.active_masks() == 0xFF).all()
    s.close()


def test_old_grid_can_go_after_regrid():
    o = random_leaves(5)
    names = COMBUST
    st = random_state(6, len(o), names)
    g, s = make_sim(o, names, st)
    s.regrid(1)
    g.reset()
    s.substep(3, 0.02, 1.0 / 32, api.CombustionParams(), False)
    s.regrid(2)
    s.substep(3, 0.02, 1.0 / 32, api.CombustionParams(), False)
    out = download(s, names)
    assert all(np.isfinite(v).all() for v in out.values())
    s.close()


def test_masks_round_trip_and_reset():
    o = random_leaves(9)
    g, s = make_sim(o, ["density"], random_state(9, len(o), ["density"]))
    assert (s.active_masks() == 0xFF).all()
    m = random_masks(10, len(o))
    s.set_active_masks(m)
    assert np.array_equal(s.active_masks(), m)
    s.set_active_masks(None)
    assert (s.active_masks() == 0xFF).all()
    s.close()


def test_refusals_leave_the_sim_as_it_was():
    o = random_leaves(11)
    names = COMBUST
    st = random_state(12, len(o), names)
    m = random_masks(13, len(o))
    g, s = make_sim(o, names, st, m)

    def unchanged():
        assert s.grid is g and np.array_equal(g.coords()[::512], o)
        assert np.array_equal(s.active_masks(), m)
        assert_same(download(s, names), st, "after a refusal")

    g.set_active_range(0, len(o) - 1)  # a multi-GPU rank's launch range
    with pytest.raises(ValueError):
        s.regrid(1)
    g.set_active_range(0, len(o))
    unchanged()
    so = np.array([[0, 0, 0]], dtype=np.int32)
    with pytest.raises(ValueError):  # an SDF source for a sim without collision_sdf
        s.regrid(1, (so, None, np.zeros(512, dtype=np.float32)))
    unchanged()
    g3, s3 = make_sim(o, names + ["collision_sdf"], {**st, "collision_sdf": st["density"]}, m)
    for bad in (np.array([[4, 0, 0]], dtype=np.int32), np.array([[8, 0, 0], [0, 0, 0], [8, 0, 0]], dtype=np.int32)):
        with pytest.raises(_lib.HNSError) as e:
            s3.regrid(1, (bad, None, np.zeros(len(bad) * 512, dtype=np.float32)))
        assert e.value.code == _lib.HNS_ERR_TOPOLOGY
        assert s3.grid is g3 and np.array_equal(s3.active_masks(), m)
    with pytest.raises(ValueError):
        s.regrid(1025)
    s.set_active_masks(np.zeros((len(o), 64), dtype=np.uint8))  # no active voxel anywhere: the SOP's "No active voxels"
    with pytest.raises(_lib.HNSError) as e:
        s.regrid(2)
    assert e.value.code == _lib.HNS_ERR_RUNTIME
    s.set_active_masks(m)
    unchanged()
    s.substep(2, 0.02, 1.0 / 32, api.CombustionParams(), False)  # still usable: it substeps and regrids
    s.regrid(1)
    assert s.grid is not g
    s.close(), s3.close()
