"""Growing a device-resident sim's domain from points on the MI355X: hns_dev_point_leaves (k_seed_keys, k_seed_compact, k_seed_masks of hns_seed.hip) against its host
mirror, hns_sim_regrid_seeded against the host chain it stands for (tests/seed_cases.py: host_chain_seeded), Sim.emit against that chain followed by the host splat mirror,
and a four-frame emitter that walks out of its domain. Every comparison is equality of bytes: the seeds are a set of keys and ORs of bits, the regrid copies and sums as
hns_sim_regrid_sourced does, the splat's sums are integers. tests/test_seed.py holds the host mirror to the numpy restatement of include/hns.h on the CPU."""
import ctypes as C

import numpy as np
import pytest

import points_cases as pc
import seed_cases as sd
from frame_cases import (COMBUST, assert_same, download, host_chain, host_deactivate, make_sim, make_sources, random_leaves, random_masks, random_state,
                         sdf_source)
from hnanosolver_amd import _lib, api, device, fields, leafio
from pool_cases import under_every_fill

pytestmark = pytest.mark.gpu

F = np.float32
N_REGRID_POINTS = 257  # of make_points' classes: far and large points bring lone leaves, which a padding of 9 turns into 5^3 each


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def regrid_points(origins, seed, n=N_REGRID_POINTS):
    xyz = pc.make_points(origins, seed, n)
    have = set(map(tuple, np.asarray(origins).tolist()))
    assert any(tuple(q) not in have for q in sd.seeds(xyz)[0].tolist()), "the seeds bring leaves the grid lacks"
    return xyz


# ---- 1. hns_dev_point_leaves ----------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,count", sd.all_point_sets(), ids=lambda v: str(v))
def test_device_seeds_equal_the_host_mirror(name, count):
    xyz = sd.point_set(name, count)
    want = leafio.point_leaves(xyz)
    t = dev(xyz)
    got = device.point_leaves(t)
    assert sd.same(got, want), f"{name}[:{count}]: {len(got[0])} leaves against {len(want[0])}, skipped {got[2]} against {want[2]}"
    assert sd.same(device.point_leaves(t), want), "second run"
    assert np.array_equal(t.cpu().numpy().view(np.uint32), xyz.view(np.uint32)), "the points are only read"
    if len(xyz) > 1:
        perm = np.random.default_rng(3).permutation(len(xyz))
        assert sd.same(device.point_leaves(dev(xyz[perm])), want), "permuted"


def test_device_query_idiom_and_refusals():
    import torch

    lib = _lib.load_library()
    xyz = sd.point_set("ball")
    want = leafio.point_leaves(xyz)
    t = dev(xyz)
    n, skipped = C.c_uint64(99), C.c_uint64(99)
    o = np.full((8, 3), 77, dtype=np.int32)
    m = np.full((8, 64), 77, dtype=np.uint8)
    assert lib.hns_dev_point_leaves(0, t.data_ptr(), len(xyz), o.ctypes.data, m.ctypes.data, 7, C.byref(n), C.byref(skipped), None) == 0
    assert n.value == 8 and skipped.value == 0 and (o == 77).all() and (m == 77).all(), "cap too small: nothing written, the count set"
    assert lib.hns_dev_point_leaves(0, t.data_ptr(), len(xyz), o.ctypes.data, None, 8, C.byref(n), None, None) == 0
    assert np.array_equal(o, want[0]) and (m == 77).all()
    for args, msg in [((0, None, 2, None, None, 0, C.byref(n), None, None), "xyz is null"),
                      ((0, t.data_ptr(), 2, None, None, 0, None, None, None), "n_leaves is null"),
                      ((0, t.data_ptr(), 2 ** 31, None, None, 0, C.byref(n), None, None), "n is above 2^31 - 1"),
                      ((torch.cuda.device_count(), t.data_ptr(), 2, None, None, 0, C.byref(n), None, None), "device")]:
        assert lib.hns_dev_point_leaves(*args) == _lib.HNS_ERR_INVALID_ARGUMENT
        text = lib.hns_last_error().decode()
        assert text.startswith("hns_dev_point_leaves:") and msg in text, text
    # a fresh grid around a particle set: every tap of every point lands
    g = api.create_grid_from_leaves(want[0], 1.0 / 32)
    status = torch.zeros(len(xyz), dtype=torch.uint8, device="cuda")
    field = torch.zeros(g.voxel_count(), dtype=torch.float32, device="cuda")
    device.splat_points(g, [field], t, [torch.ones(len(xyz), dtype=torch.float32, device="cuda")], status=status)
    assert (status.cpu().numpy() == 8).all()


# ---- 2. the seeded regrid against the host chain -----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("null_masks", [False, True], ids=["masks", "nullmasks"])
@pytest.mark.parametrize("kind", ["none", "velocity", "mixed"])
@pytest.mark.parametrize("with_sdf", [False, True], ids=["nosdf", "sdf"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_seeded_regrid_matches_the_host_chain(p, with_sdf, kind, null_masks):
    names = COMBUST + (["collision_sdf"] if with_sdf else [])
    seed = 17 * p + 5 * with_sdf + len(kind) + 3 * null_masks
    o = random_leaves(seed)
    m = None if null_masks else random_masks(seed + 1, len(o))
    st = random_state(seed + 2, len(o), names)
    g, s = make_sim(o, names, st, m)
    sdf = sdf_source(seed + 3, o) if with_sdf else None
    src = None if kind == "none" else make_sources(seed + 4, o, kind, "straddling")
    xyz = regrid_points(o, seed)
    ng = s.regrid(p, sdf, src, points=dev(xyz))
    dom, dm, want = sd.host_chain_seeded(o, m, st, names, p, xyz, src, sdf)
    dom0 = host_chain(o, m, st, names, p, src, sdf)[0]
    assert len(dom) > len(dom0), "the seeds grew the domain"
    assert s.grid is ng and ng.ptr != g.ptr and g.leaf_count() == len(o)
    assert np.array_equal(ng.coords()[::512], dom), "leaf set / OpenVDB order"
    assert np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"p={p} {kind} sdf={with_sdf}")  # (as bytes: the -0.0f of an unsourced field stay)
    assert s.last_seeds_skipped == 0
    t = s.regrid_times()
    assert set(t) == {"candidates", "host", "masks", "fields"} and all(v >= 0 for v in t.values())
    s.close()


def test_velocity_keeps_its_negative_zeros_where_the_host_detour_loses_them():
    names = COMBUST
    o = random_leaves(71)
    st = random_state(72, len(o), names)
    g, s = make_sim(o, names, st)
    xyz = regrid_points(o, 71)
    s.regrid(1, points=dev(xyz))
    got = download(s, names)
    neg = lambda v: int(((v.view(np.uint32) == 0x80000000)).sum())
    assert neg(got["vel"]) == neg(st["vel"]) > 0
    so, sm, _ = sd.seeds(xyz)
    detour = host_chain(o, None, st, names, 1, {"vel": (so, sm, np.zeros((len(so) * 512, 3), F))})[2]
    assert neg(detour["vel"]) == 0, "the empty velocity source of the host detour turns every -0.0f into +0.0f"
    s.close()


def test_skipped_points_are_counted_and_seed_nothing():
    names = COMBUST
    o = random_leaves(73)
    st = random_state(74, len(o), names)
    g, s = make_sim(o, names, st)
    xyz = sd.point_set("edges")
    s.regrid(0, points=dev(xyz))
    dom, dm, want = sd.host_chain_seeded(o, None, st, names, 0, xyz)
    assert s.last_seeds_skipped == sd.seeds(xyz)[2] > 0
    assert np.array_equal(s.grid.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "edges")
    s.close()


# ---- 3. no points ------------------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["none", "mixed"])
def test_zero_points_is_the_unseeded_regrid(kind):
    import torch

    names = COMBUST + ["collision_sdf"]
    o = random_leaves(31)
    m = random_masks(32, len(o))
    st = random_state(33, len(o), names)
    sdf = sdf_source(34, o)
    src = None if kind == "none" else make_sources(35, o, kind, "straddling")
    g1, s1 = make_sim(o, names, st, m)
    g2, s2 = make_sim(o, names, st, m)
    a = s1.regrid(2, sdf, src)
    b = s2.regrid(2, sdf, src, points=torch.empty((0, 3), dtype=torch.float32, device="cuda"))
    assert np.array_equal(a.coords(), b.coords())
    assert np.array_equal(s1.active_masks(), s2.active_masks())
    assert_same(download(s1, names), download(s2, names), "zero points")
    assert s2.last_seeds_skipped == 0
    s1.close(), s2.close()


# ---- 4. a sim with nothing active restarts from points -------------------------------------------------------------------------------------------------------------------------


def test_cleared_masks_restart_from_one_point():
    names = COMBUST
    o = random_leaves(61)
    st = random_state(62, len(o), names)
    zero = np.zeros((len(o), 64), np.uint8)
    g, s = make_sim(o, names, st, zero)
    with pytest.raises(_lib.HNSError, match="No active voxels") as e:
        s.regrid(1)
    assert e.value.code == _lib.HNS_ERR_RUNTIME
    assert s.grid is g and np.array_equal(s.active_masks(), zero)
    assert_same(download(s, names), st, "after the refused regrid")
    point = (o[0].astype(np.float64) + np.array([7.5, 3.25, 0.0])).astype(F).reshape(1, 3)  # inside an old leaf, astride its +x face, on its -z face
    ng = s.regrid(1, points=dev(point))
    so, sm, _ = sd.seeds(point)
    want_o, want_m = leafio.dilate_leaf_masks(so, 1, sm)
    assert np.array_equal(ng.coords()[::512], want_o) and np.array_equal(s.active_masks(), want_m), "the dilation of the point's eight taps"
    dom, dm, want = sd.host_chain_seeded(o, zero, st, names, 1, point)
    assert np.array_equal(dom, want_o) and np.array_equal(dm, want_m)
    got = download(s, names)
    assert_same(got, want, "restart")
    assert all(not v.any() for v in got.values()), "the unseeded regrid holds nothing: no value comes back with the leaves"
    s.close()


# ---- 5. emit -----------------------------------------------------------------------------------------------------------------------------------------------------------------


def host_emit(origins, masks, state, names, p, xyz, values, velocity, vs, sources=None, sdf=None):
    """host_chain_seeded, then the host splat mirror with activate on the new grid -> (origins, masks, state, status)"""
    dom, dm, st = sd.host_chain_seeded(origins, masks, state, names, p, xyz, sources, sdf)
    hg = api.create_grid_from_leaves(dom, vs)
    targets = [st[k] for k in values] + ([st["vel"]] if velocity is not None else [])
    status = np.zeros(len(xyz), dtype=np.uint8)
    dm = np.ascontiguousarray(dm)
    api.splat_points_host(hg, targets, xyz, list(values.values()) + ([velocity] if velocity is not None else []), masks=dm, activate=True, status=status)
    return dom, dm, st, status


@pytest.mark.parametrize("name", ["ragged32", "sparse_far"])
def test_emit_lands_every_tap_and_matches_the_host(name):
    names = COMBUST
    vs = 1.0 / 32
    o, _, _, pts = pc.case(name)
    xyz = np.ascontiguousarray(np.concatenate([pts[:1025], sd.point_set("edges"), sd.point_set("ball")[:513]]))
    rng = np.random.default_rng([9, len(o)])
    m = random_masks(5, len(o))
    st = random_state(6, len(o), names)
    values = {k: rng.standard_normal(len(xyz)).astype(F) for k in ("density", "fuel")}
    velocity = rng.standard_normal((len(xyz), 3)).astype(F)
    g, s = make_sim(o, names, st, m, vs)
    grid, status = s.emit({k: dev(v) for k, v in values.items()}, dev(xyz), dev(velocity), padding=1)
    dom, dm, want, want_status = host_emit(o, m, st, names, 1, xyz, values, velocity, vs)
    status = status.cpu().numpy()
    seeding = sd.seeding(xyz)
    assert (status[seeding] == 8).all(), "every tap of every seeding point landed"
    assert np.array_equal(status, want_status) and s.last_seeds_skipped == int((~seeding).sum()) > 0
    assert grid is s.grid and np.array_equal(grid.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, f"{name}: emit")
    hg, hs = make_sim(dom, names, want, dm, vs)
    for sim in (s, hs):
        for _ in range(2):
            sim.substep(4, 1.0 / 24, vs, api.CombustionParams(), False)
    assert_same(download(s, names), download(hs, names), f"{name}: two substeps after emit")
    s.close(), hs.close()


# ---- 6. an emitter that walks out of its domain ----------------------------------------------------------------------------------------------------------------------------------


def test_four_frame_emitter_walks_out_through_a_face():
    R, names, vs = 32, COMBUST, 1.0 / 32
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + names}
    g, s = make_sim(o, names, st, None, vs)
    grids = [g]
    ho, hm, hst = o, None, st
    params = api.CombustionParams()
    tolerances, vtol = {"density": 0.02}, 0.02
    for frame in range(4):
        xyz = sd.emitter_ball((24 + 7 * frame, 16, 16), seed=frame)  # the +x face is at x = 32: inside, astride, outside, a leaf beyond
        rng = np.random.default_rng(200 + frame)
        values = {k: rng.random(len(xyz)).astype(F) for k in ("density", "temperature", "fuel")}
        velocity = (rng.random((len(xyz), 3)) * F(0.5)).astype(F)
        grid, status = s.emit({k: dev(v) for k, v in values.items()}, dev(xyz), dev(velocity), padding=1)
        grids.append(grid)
        ho, hm, hst, want_status = host_emit(ho, hm, hst, names, 1, xyz, values, velocity, vs)
        assert (status.cpu().numpy() == 8).all() and (want_status == 8).all(), f"frame {frame}: a tap was dropped"
        assert np.array_equal(s.grid.coords()[::512], ho) and np.array_equal(s.active_masks(), hm), f"frame {frame} regrid"
        assert_same(download(s, names), hst, f"frame {frame} emit")
        hg, hs = make_sim(ho, names, hst, None, vs)
        for sim in (s, hs):
            for _ in range(2):
                sim.substep(4, 1.0 / 24, vs, params, False)
        hst = download(hs, names)
        hs.close()
        counts = s.deactivate(tolerances, vtol, counts=True)
        hm, hc = host_deactivate(hm, hst, tolerances, vtol)
        assert counts == hc and np.array_equal(s.active_masks(), hm), f"frame {frame} deactivate"
        assert_same(download(s, names), hst, f"frame {frame}")
    assert len(ho) > len(o) and ho[:, 0].max() >= 48, "the domain followed the emitter out"
    s.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------------


def raw_seeded(sim, p, entries, xyz_ptr, n_seeds):
    """hns_sim_regrid_seeded with hand-built hns_leaf_source entries (name, ncomp, origins, values) -> (grid ptr, err, message, skipped)"""
    lib = _lib.load_library()
    arr = (_lib.hns_leaf_source * max(1, len(entries)))()
    keep = []
    for i, (name, nc, o, v) in enumerate(entries):
        b = name.encode()
        keep += [b, o, v]
        arr[i].name, arr[i].ncomp, arr[i].n_leaves = b, nc, len(o)
        arr[i].origins, arr[i].masks, arr[i].values = o.ctypes.data, None, v.ctypes.data
    err, skipped = C.c_int(0), C.c_uint64(99)
    ptr = lib.hns_sim_regrid_seeded(sim._ptr, p, arr, len(entries), xyz_ptr, n_seeds, C.byref(skipped), None, 0, None, None, None, C.byref(err))
    return ptr, err.value, lib.hns_last_error().decode(), skipped.value


def test_refusals_leave_the_sim_as_it_was():
    names = COMBUST
    o = random_leaves(51)
    st = random_state(52, len(o), names)
    m = random_masks(53, len(o))
    g, s = make_sim(o, names, st, m)

    def unchanged():
        assert s.grid is g and np.array_equal(g.coords()[::512], o)
        assert np.array_equal(s.active_masks(), m)
        assert_same(download(s, names), st, "after a refusal")

    xyz = regrid_points(o, 51)
    t = dev(xyz)
    one, v1 = np.array([[0, 0, 0]], dtype=np.int32), np.ones(512, dtype=F)
    far = np.array([[800, 0, 0], [800, 0, 0]], dtype=np.int32)
    cases = [
        (([], None, 5), _lib.HNS_ERR_INVALID_ARGUMENT, "d_seed_xyz is null"),
        (([], t.data_ptr(), 2 ** 31), _lib.HNS_ERR_INVALID_ARGUMENT, "n_seeds is above 2^31 - 1"),
        (([("smoke", 1, one, v1)], t.data_ptr(), len(xyz)), _lib.HNS_ERR_INVALID_ARGUMENT, "no float field 'smoke'"),
        (([("fuel", 1, far, np.ones(2 * 512, dtype=F))], t.data_ptr(), len(xyz)), _lib.HNS_ERR_TOPOLOGY, "duplicate leaf origin"),
    ]
    for (entries, ptr, n), code, msg in cases:
        got, err, text, skipped = raw_seeded(s, 1, entries, ptr, n)
        assert not got and err == code, (msg, err, text)
        assert msg in text and text.startswith("hns_sim_regrid_seeded:"), text
        unchanged()
    # 2^19 + 1 points on leaf corners 16 voxels apart: eight leaves each, none shared, so the new domain exceeds 2^22 leaves at p = 0
    k = np.arange(2 ** 19 + 1, dtype=np.int64)
    corners = np.stack([k % 81, (k // 81) % 81, k // (81 * 81)], axis=1)
    big = np.ascontiguousarray((corners * 16 + 7.5).astype(F))
    with pytest.raises(_lib.HNSError, match="exceeds the 2\\^22-leaf") as e:
        s.regrid(0, points=dev(big))
    assert e.value.code == _lib.HNS_ERR_TOPOLOGY
    unchanged()
    s.regrid(1, points=t)  # still usable: a good seeded regrid afterwards matches the host chain
    dom, dm, want = sd.host_chain_seeded(o, m, st, names, 1, xyz)
    assert np.array_equal(s.grid.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "after the refusals")
    s.close()


# ---- 8. pooled scratch -----------------------------------------------------------------------------------------------------------------------------------------------------------


def pool_scenario():
    names = COMBUST + ["collision_sdf"]
    o = random_leaves(81)
    m = random_masks(82, len(o))
    st = random_state(83, len(o), names)
    xyz = regrid_points(o, 81)
    out = {}
    for label, pts in (("points", xyz), ("ball", sd.point_set("ball")), ("edges", sd.point_set("edges"))):
        got = device.point_leaves(dev(pts))
        assert sd.same(got, leafio.point_leaves(pts)), label
        out.update({f"{label}/origins": got[0], f"{label}/masks": got[1], f"{label}/skipped": got[2]})
    g, s = make_sim(o, names, st, m)
    for frame, p in enumerate((1, 9)):
        s.regrid(p, sdf_source(84 + frame, o), make_sources(86 + frame, o, "mixed", "straddling"), points=dev(xyz))
        out.update({f"regrid{frame}/origins": s.grid.coords()[::512], f"regrid{frame}/masks": s.active_masks()})
        out.update({f"regrid{frame}/{k}": v for k, v in download(s, names).items()})
    s.close()
    return out


def test_results_do_not_depend_on_what_the_pooled_scratch_held():
    under_every_fill(pool_scenario)
