"""Points rasterised into fields on the GPU: hns_dev_splat_points and hns_sim_splat_points under a stored spec (k_splat_radial<1 | 4 | 16 | 64> of hns_rasterize.hip, the
weight channel of k_splat_points and the average form of k_splat_finish in hns_splat.hip) and their Python keywords.

Every comparison is equality of bytes against the host mirror hns_grid_splat_points_spec, which tests/test_rasterize.py holds to the numpy restatement of include/hns.h on
the CPU: fields, status, the rejected count, masks. There is no tolerance: the sums are integers. Grids, points, radii and the conditions they meet: tests/rasterize_cases.py."""
import functools
import time

import numpy as np
import pytest

import points_cases as pc
import rasterize_cases as rc
import seed_cases as sd
import splat_cases as sp
import stream_cases as stc
from frame_cases import LAUNCH_RANGES, assert_same, download, launch_range, make_sim, random_masks, random_state

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 24.0
SENTINEL = 0xAB
REJECTED_BEFORE = 5
MODES = ("add", "average")


class Rig:
    """a device grid over a leaf set (the host mirror runs on the same grid)"""

    def __init__(self, origins):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.grid = api.create_grid_from_leaves(np.ascontiguousarray(origins, dtype=np.int32), VS)

    def dev(self, a):
        return self.t.from_numpy(np.array(a)).cuda()

    def padded(self, a, fill=7.0):
        """(device tensor one row longer than a, its first len(a) rows): no call gets a null pointer for n = 0, and the row behind the last is watched"""
        a = np.asarray(a)
        full = self.t.full((len(a) + 1, *a.shape[1:]), fill, dtype=self.t.float32, device="cuda")
        full[: len(a)] = self.dev(a)
        return full, full[: len(a)]

    def splat(self, fields, xyz, values, q=-32, what="", per_point=None, **spec):
        """one hns_dev_splat_points call under the spec, on copies -> (new fields, status, rejected); the inputs and the byte behind the last status are watched"""
        n = len(xyz)
        d_fields = [self.dev(f) for f in fields]
        watched = [self.padded(np.asarray(xyz, dtype=F).reshape(-1, 3))] + [self.padded(v) for v in values]
        originals = [np.asarray(xyz, dtype=F).reshape(-1, 3)] + list(values)
        if per_point is not None:
            watched.append(self.padded(per_point))
            originals.append(per_point)
            spec = dict(spec, radius=watched[-1][1], max_radius=spec["radius"])
        status = self.t.full((n + 1,), SENTINEL, dtype=self.t.uint8, device="cuda")
        rejected = self.t.full((1,), REJECTED_BEFORE, dtype=self.t.int64, device="cuda")
        self.D.splat_points(self.grid, d_fields, watched[0][1], [w[1] for w in watched[1 : 1 + len(values)]], q, status[:n], rejected, **spec)
        st = status.cpu().numpy()
        assert st[n] == SENTINEL, f"{what}: status was written behind its last byte"
        for (full, _), a in zip(watched, originals):
            assert sp.same_bytes(full.cpu().numpy()[:n], a) and (full.cpu().numpy()[n:] == 7.0).all(), f"{what}: an input changed"
        return [f.cpu().numpy() for f in d_fields], st[:n], int(rejected.cpu().numpy()[0]) - REJECTED_BEFORE


@functools.lru_cache(maxsize=None)
def rig(name):
    rc.oracle_grid(name)  # (asserts the case's conditions)
    return Rig(rc.case(name)[0])


def assert_equal_the_mirror(R, fields, xyz, values, q, what, per_point=None, **spec):
    got, status, rej = R.splat(fields, xyz, values, q, what, per_point, **spec)
    host = dict(spec, radius=per_point, max_radius=spec["radius"]) if per_point is not None else spec
    want, want_status, want_rej, _ = rc.mirror(R.grid, fields, xyz, values, q, **host)
    for i in range(len(fields)):
        d = np.flatnonzero(got[i].reshape(-1).view(np.uint32) != want[i].reshape(-1).view(np.uint32))
        assert len(d) == 0, f"{what}: field {i}: {len(d)} words differ, first at {d[:6].tolist()}"
        assert not want_status.any() or not sp.same_bytes(got[i], fields[i]), f"{what}: field {i}: nothing changed"  # (where the mirror says that a point landed)
    assert sp.same_bytes(status, want_status), f"{what}: status"
    assert rej == want_rej, f"{what}: rejected {rej} against {want_rej}"
    return got, status


# ---------------------------------------------------------------------------------------------------------------
# 1. the device equals the host mirror
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", rc.COUNTS)
@pytest.mark.parametrize("name", rc.GRIDS)
def test_device_equals_the_mirror(name, n):
    """one radius per group size, both modes, a float and a Vec3f target (four components: one pass of a sum, two of an average)"""
    R, (_, vel, phi, xyz, vals, vvals, _, _) = rig(name), rc.case(name)
    for G, radius in rc.GROUP_RADII.items():
        for mode in MODES:
            assert_equal_the_mirror(R, [phi[0], vel], xyz[:n], [vals[0][:n], vvals[:n]], -32, f"{name} n={n} G={G} {mode}", kernel="radial", mode=mode, radius=radius)
    assert_equal_the_mirror(R, [phi[0], vel], xyz[:n], [vals[0][:n], vvals[:n]], -32, f"{name} n={n} trilinear average", kernel="trilinear", mode="average", min_weight=0.25)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rc.GRIDS)
def test_seven_components_and_every_quantum(name, mode):
    """four floats and the velocity: two passes of a sum, three of an average, each with its own weight channel"""
    R, (_, vel, phi, xyz, vals, vvals, _, _) = rig(name), rc.case(name)
    for q, radius in zip(sp.QUANTA, (2.5, 1.0, 4.0)):
        assert_equal_the_mirror(R, phi[:4] + [vel], xyz, vals[:4] + [vvals], q, f"{name} seven components {mode} Q={q} r={radius}", kernel="radial", mode=mode, radius=radius,
                                min_weight=0.125 if mode == "average" else 0.0)


@pytest.mark.parametrize("bound", (4.0, 2.5, 0.5))
def test_one_radius_per_point_with_the_special_values(bound):
    """0, -1, NaN, +inf, a subnormal, 4.0f and the float above it among the radii: what does not rasterise lands nowhere, the bound decides the group of lanes"""
    R, (_, vel, phi, xyz, vals, vvals, _, radii) = rig("ragged32"), rc.case("ragged32")
    for mode in MODES:
        _, status = assert_equal_the_mirror(R, [phi[0], vel], xyz, [vals[0], vvals], -32, f"per-point radii, bound {bound}, {mode}", per_point=radii, kernel="radial", mode=mode,
                                            radius=bound)
        with np.errstate(invalid="ignore"):
            refused = ~((radii > 0) & (radii <= F(bound)))
        assert refused.sum() >= 20 and (status[refused] == 0).all() and (status[~refused] == 2).any()


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_footprints_land_in_every_leaf_whatever_the_launch_range(kind):
    """include/hns.h: a footprint voxel lands in a leaf whatever the grid's launch range, ghost leaves included -- a radial sum and a radial average give the bytes of the
    whole range, which equal the mirror, under set_active_range on a strict inner range and under set_active_leaves(n // 2)"""
    R, (_, vel, phi, xyz, vals, vvals, _, _) = rig("ragged32"), rc.case("ragged32")
    for mode in MODES:
        kw = dict(kernel="radial", mode=mode, radius=2.5, min_weight=0.125 if mode == "average" else 0.0)
        whole, whole_status = assert_equal_the_mirror(R, [phi[0], vel], xyz, [vals[0], vvals], -32, f"whole range, {mode}", **kw)
        _, _, whole_rejected = R.splat([phi[0], vel], xyz, [vals[0], vvals], -32, f"whole range, {mode}", **kw)
        with launch_range(R.grid, kind):
            got, status, rejected = R.splat([phi[0], vel], xyz, [vals[0], vvals], -32, f"{kind}, {mode}", **kw)
        assert R.grid.active_leaves() == R.grid.leaf_count()
        assert sp.same_bytes(got[0], whole[0]) and sp.same_bytes(got[1], whole[1]), f"{kind}, {mode}: a field differs from the whole range's"
        assert sp.same_bytes(status, whole_status) and rejected == whole_rejected, f"{kind}, {mode}: status or rejected"


# ---------------------------------------------------------------------------------------------------------------
# 2. order, repetition, contention
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
def test_a_permuted_point_order_and_a_second_run_give_the_same_bytes(mode):
    R, (_, vel, phi, xyz, vals, vvals, _, _) = rig("dense32"), rc.case("dense32")
    kw = dict(kernel="radial", mode=mode, radius=2.5)
    first, status = assert_equal_the_mirror(R, [phi[0], vel], xyz, [vals[0], vvals], -32, f"in order, {mode}", **kw)
    again, _, _ = R.splat([phi[0], vel], xyz, [vals[0], vvals], -32, "again", **kw)
    p = np.random.default_rng(5).permutation(len(xyz))
    permuted, pstatus, _ = R.splat([phi[0], vel], xyz[p], [vals[0][p], vvals[p]], -32, "permuted", **kw)
    for i in range(2):
        assert sp.same_bytes(first[i], again[i]), f"{mode}: two runs differ in field {i}"
        assert sp.same_bytes(first[i], permuted[i]), f"{mode}: the point order changed field {i}"
    assert sp.same_bytes(status[p], pstatus)


@pytest.mark.parametrize("mode", MODES)
def test_contended_footprints_equal_the_mirror(mode):
    """4,099 points in one cell at r = 4: every voxel of a 9^3 neighbourhood receives thousands of terms per channel"""
    R, (_, vel, phi, _, _, _, _, _) = rig("dense32"), rc.case("dense32")
    rng = np.random.default_rng(17)
    xyz = (np.array([13.0, 7.0, 22.0]) + rng.uniform(0.0, 1.0, (4099, 3))).astype(F)
    vals, vvals = (rng.standard_normal(len(xyz)) * 3.0).astype(F), (rng.standard_normal((len(xyz), 3)) * 3.0).astype(F)
    _, status = assert_equal_the_mirror(R, [phi[0], vel], xyz, [vals, vvals], -32, f"contended {mode}", kernel="radial", mode=mode, radius=4.0)
    assert (status == 2).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. Sim.splat and Sim.emit
# ---------------------------------------------------------------------------------------------------------------

SIM_NAMES = ["density", "fuel", "collision_sdf"]


@pytest.mark.parametrize("activate", (True, False))
def test_sim_splat_equals_the_mirror_and_leaves_the_default_path_as_it_was(activate):
    import torch

    from hnanosolver_amd import _lib

    o, _, _, xyz, vals, vvals, masks, radii = rc.case("ragged32")
    state = random_state(13, len(o), SIM_NAMES)
    g, s = make_sim(o, SIM_NAMES, state, np.array(masks), VS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    p = dev(xyz)
    now, m_now = download(s, SIM_NAMES), s.active_masks()
    # an average of two float fields and the velocity with one radius per point, then a radial sum at another radius
    kw = dict(kernel="radial", mode="average", min_weight=0.5)
    st = s.splat({"fuel": dev(vals[0]), "density": dev(vals[1])}, p, velocity=dev(vvals), activate=activate, status=True, radius=dev(radii), max_radius=4.0, **kw)
    want, want_status, _, want_masks = rc.mirror(g, [now["fuel"], now["density"], now["vel"]], xyz, [vals[0], vals[1], vvals], -32, m_now, activate, radius=radii, max_radius=4.0, **kw)
    assert sp.same_bytes(st.cpu().numpy(), want_status) and set(np.unique(want_status).tolist()) == {0, 1, 2}
    assert s.splat({"density": dev(vals[2])}, p, log2_quantum=-24, activate=activate, kernel="radial", radius=1.5) is None
    want2, _, _, want_masks = rc.mirror(g, [want[1]], xyz, [vals[2]], -24, want_masks, activate, kernel="radial", mode="add", radius=1.5)
    expect = {"vel": want[2], "density": want2[0], "fuel": want[0], "collision_sdf": now["collision_sdf"]}
    assert_same(download(s, SIM_NAMES), expect, "Sim.splat under a spec")
    assert sp.same_bytes(s.active_masks(), want_masks) and sp.same_bytes(want_masks, m_now) == (not activate)
    # the keywords put the sim's spec back: a call without them is the trilinear sum of before, from a clean accumulator
    spec = _lib.hns_splat_spec(9, 9, 9.0, 9, 9.0)
    assert _lib.lib.hns_sim_get_splat_spec(s._ptr, spec) == 0 and (spec.kernel, spec.mode, spec.radius, spec.d_radius, spec.min_weight) == (0, 0, 0.0, None, 0.0)
    st = s.splat({"fuel": dev(vals[3])}, p, velocity=dev(vvals), activate=activate, status=True)
    want3, want_status3, _, want_m3 = sp.mirror(g, [expect["fuel"], expect["vel"]], xyz, [vals[3], vvals], -32, want_masks, activate)
    after = download(s, SIM_NAMES)
    assert sp.same_bytes(after["fuel"], want3[0]) and sp.same_bytes(after["vel"], want3[1]) and sp.same_bytes(after["density"], expect["density"])
    assert sp.same_bytes(st.cpu().numpy(), want_status3) and sp.same_bytes(s.active_masks(), want_m3)
    s.close()


def test_a_stored_spec_is_what_the_plain_calls_read_and_a_sim_keeps_it_across_a_regrid():
    import ctypes as C

    import torch

    from hnanosolver_amd import _lib

    lib = _lib.load_library()
    o, _, _, xyz, vals, _, masks, _ = rc.case("ragged32")
    state = random_state(3, len(o), SIM_NAMES)
    g, s = make_sim(o, SIM_NAMES, state, np.array(masks), VS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    spec = _lib.hns_splat_spec(1, 1, 1.5, None, 0.0)
    assert lib.hns_sim_set_splat_spec(s._ptr, C.byref(spec)) == 0
    grid = s.regrid(1)
    got = _lib.hns_splat_spec()
    assert lib.hns_sim_get_splat_spec(s._ptr, C.byref(got)) == 0 and (got.kernel, got.mode, got.radius) == (1, 1, 1.5)
    now, m_now = download(s, SIM_NAMES), s.active_masks()
    names = (C.c_char_p * 1)(b"density")
    v, p = dev(vals[0]), dev(xyz)
    status = torch.full((len(xyz),), SENTINEL, dtype=torch.uint8, device="cuda")
    assert lib.hns_sim_splat_points(s._ptr, names, 1, None, p.data_ptr(), (C.c_void_p * 1)(v.data_ptr()), len(xyz), -32, 1, status.data_ptr(), None, None) == 0
    want, want_status, _, want_masks = rc.mirror(grid, [now["density"]], xyz, [vals[0]], -32, m_now, True, kernel="radial", mode="average", radius=1.5)
    assert sp.same_bytes(download(s, SIM_NAMES)["density"], want[0]) and sp.same_bytes(status.cpu().numpy(), want_status) and sp.same_bytes(s.active_masks(), want_masks)
    s.close()


def test_emit_with_a_radius_lands_every_footprint_and_matches_the_host_chain():
    import torch

    from hnanosolver_amd import api

    names, vs = ["density", "fuel"], 1.0 / 32
    o, _, _, pts = pc.case("ragged32")
    xyz = np.ascontiguousarray(np.concatenate([pts[:1025], sd.point_set("edges"), sd.point_set("ball")[:513]]))
    rng = np.random.default_rng([9, len(o)])
    m, st = random_masks(5, len(o)), random_state(6, len(o), names)
    values = {k: rng.standard_normal(len(xyz)).astype(F) for k in names}
    velocity = rng.standard_normal((len(xyz), 3)).astype(F)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    g, s = make_sim(o, names, st, m, vs)
    with pytest.raises(ValueError, match="padding >= ceil"):
        s.emit({k: dev(v) for k, v in values.items()}, dev(xyz), dev(velocity), padding=2, radius=2.5)
    assert s.grid is g, "a refused emit ran its regrid"
    grid, status = s.emit({k: dev(v) for k, v in values.items()}, dev(xyz), dev(velocity), padding=3, radius=2.5, mode="average")
    dom, dm, want = sd.host_chain_seeded(o, m, st, names, 3, xyz, None, None)
    hg, dm = api.create_grid_from_leaves(dom, vs), np.ascontiguousarray(dm)
    want_status = np.zeros(len(xyz), dtype=np.uint8)
    api.splat_points_host(hg, [want[k] for k in names] + [want["vel"]], xyz, list(values.values()) + [velocity], masks=dm, activate=True, status=want_status, kernel="radial",
                          mode="average", radius=2.5)
    status, seeding = status.cpu().numpy(), sd.seeding(xyz)
    assert seeding.sum() > 1000 and (status[seeding] == 2).all(), "every footprint voxel of every seeding point landed"
    assert np.array_equal(status, want_status) and (status[~seeding] == 0).all()
    assert np.array_equal(grid.coords()[::512], dom) and np.array_equal(s.active_masks(), dm)
    assert_same(download(s, names), want, "emit with a radius")
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. late on a non-blocking stream
# ---------------------------------------------------------------------------------------------------------------


def test_a_radial_average_late_on_a_non_blocking_stream():
    """positions, values, radii and the fields arrive behind a delay on the stream of the call; the spec is set and put back on the host while the launches wait"""
    import torch

    R, (_, vel, phi, xyz, vals, vvals, _, radii) = rig("ragged32"), rc.case("ragged32")
    n = len(xyz)
    kw = dict(kernel="radial", mode="average", min_weight=0.25)
    want, want_status, want_rej, _ = rc.mirror(R.grid, [phi[0], vel], xyz, [vals[0], vvals], -32, radius=radii, max_radius=4.0, **kw)
    host = {"density": phi[0], "vel": vel, "xyz": xyz, "vals": vals[0], "vals3": vvals, "radii": radii, "rejected": np.zeros(1, np.int64)}
    staging = {k: torch.from_numpy(np.array(v)).pin_memory() for k, v in host.items()}
    t = {k: torch.empty_like(v, device="cuda") for k, v in staging.items()}
    status = torch.empty(n, dtype=torch.uint8, device="cuda")

    def fn(stream):
        R.D.splat_points(R.grid, [t["density"], t["vel"]], t["xyz"], [t["vals"], t["vals3"]], status=status, rejected=t["rejected"], radius=t["radii"], max_radius=4.0, **kw)

    for k in t:
        t[k].copy_(staging[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(None)  # (the host time of one call, and the kernels loaded)
    host_seconds = time.perf_counter() - t0
    delay = stc.Delay(torch)
    inputs = {k: stc.Operand(t[k], staging[k], torch.full((1,), 12345, dtype=torch.int64, device="cuda") if k == "rejected" else None) for k in t}
    late = stc.late_call(fn, inputs, {"density": t["density"], "vel": t["vel"], "rejected": t["rejected"], "status": status}, delay, delay.for_host_time(host_seconds), True, None,
                         "radial average")
    stc.assert_inputs_unchanged(late.inputs, staging, inplace=("density", "vel", "rejected"), what="radial average")
    assert sp.same_bytes(late.outputs["density"].cpu().numpy(), want[0]) and sp.same_bytes(late.outputs["vel"].cpu().numpy(), want[1])
    assert sp.same_bytes(late.outputs["status"].cpu().numpy(), want_status) and int(late.outputs["rejected"].cpu()[0]) == want_rej
