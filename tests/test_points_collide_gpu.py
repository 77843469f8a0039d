"""Points traced against a collision SDF on the GPU: hns_dev_trace_points_collide / hns_sim_trace_points_collide (k_trace_points_collide of hns_points_collide.hip) and
their Python mirrors, against the numpy mirror of tests/points_collide_cases.py, which restates include/hns.h on the oracle's samplers.

Every comparison is equality of 32-bit words for positions and of bytes for status and hit; a NaN counts as equal to any NaN only in the special-value test, as in
tests/test_points_gpu.py. Every output is made one row (one byte) longer than asked and the element behind the last is watched. The conditions the point sets meet -- how
many points start inside, are put back, killed, pushed out by the first or a later push -- are held without a GPU by tests/test_points_collide_cases.py. The two entry
points run late on a non-blocking stream inside guard bands at the end of this file, with the harness and the cases of tests/stream_cases.py (tests/test_streams_gpu.py runs
the same two entries of its table; here they stand next to the feature's other tests)."""
import functools

import numpy as np
import pytest

import points_cases as pc
import points_collide_cases as cc
import special_cases as sc
from frame_cases import download, make_sim, random_masks, random_state
from oracle_lib import OracleGrid, oracle_device
from test_points_gpu import SENTINEL, STATUS_SENTINEL, Rig, assert_same_bits, assert_words, rig, words

pytestmark = pytest.mark.gpu

F = np.float32
SPEC = dict(threshold=cc.THRESHOLD, skin=cc.SKIN, iterations=cc.ITERATIONS)


@functools.lru_cache(maxsize=None)
def dev_sdf(name, variant):
    return rig(name).dev(cc.sdf_of(name, variant))


def trace_collide(R, vel, sdf, xyz, dt, inv_dx, order, steps, mode, what="", **spec):
    """-> (positions, status, hit) of one hns_dev_trace_points_collide call; the row and the bytes behind the last point are watched"""
    n = len(xyz)
    pfull, p = R.points(xyz)
    st = R.t.full((n + 1,), STATUS_SENTINEL, dtype=R.t.uint8, device="cuda")
    ht = R.t.full((n + 1,), STATUS_SENTINEL, dtype=R.t.uint8, device="cuda")
    R.D.trace_points_collide(R.grid, vel, sdf, p, dt, inv_dx, order, steps, mode=mode, status=st[:n], hit=ht[:n], **{**SPEC, **spec})
    got, status, hit = pfull.cpu().numpy(), st.cpu().numpy(), ht.cpu().numpy()
    assert (words(got[n:]) == 0xDEADBEEF).all() and status[n] == STATUS_SENTINEL and hit[n] == STATUS_SENTINEL, f"{what}: written behind the last point"
    return got[:n], status[:n], hit[:n]


def check(R, G, vel_np, sdf_np, sdf_dev, xyz, dt, order, steps, mode, what, same=assert_words, n_list=None, **spec):
    want, status, hit, cls = cc.collide_mirror(G, vel_np, sdf_np, xyz, dt, pc.INV_DX, order, steps, mode, **{**SPEC, **spec})
    u = R.dev(vel_np)
    for n in n_list or (len(xyz),):
        got, st, ht = trace_collide(R, u, sdf_dev, xyz[:n], dt, pc.INV_DX, order, steps, mode, what, **spec)
        same(got, want[:n], f"{what} n={n}: positions")
        assert np.array_equal(st, status[:n]), f"{what} n={n}: status differs at {np.flatnonzero(st != status[:n])[:6].tolist()}"
        assert np.array_equal(ht, hit[:n]), f"{what} n={n}: hit differs at {np.flatnonzero(ht != hit[:n])[:6].tolist()}: {ht[ht != hit[:n]][:6]} vs {hit[:n][ht != hit[:n]][:6]}"
    return want, status, hit, cls


@pytest.mark.parametrize("speed", pc.SPEEDS)
@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("name", pc.GRIDS)
def test_traces_equal_the_mirror(name, order, speed):
    """the full 4,099 points over modes, signs of dt, 1 and 3 steps and both SDF variants"""
    o, vel, _, xyz = pc.case(name)
    R, G = rig(name), OracleGrid(o)
    seen = dict.fromkeys(("reverted", "killed", "first_push", "later_push", "push_reverted"), 0)
    for variant in cc.VARIANTS:
        for dt in (pc.DT, -pc.DT):
            u = pc.scaled_velocity(vel, speed, F(dt) * F(pc.INV_DX))
            for steps in (1, 3):
                for mode in cc.MODES:
                    what = f"{name} {variant} order {order} speed {speed} dt {dt} steps {steps} {mode}"
                    want, status, hit, cls = check(R, G, u, cc.sdf_of(name, variant), dev_sdf(name, variant), xyz, dt, order, steps, mode, what)
                    c = cc.classes(xyz, want, hit, cls)
                    for k in seen:
                        seen[k] += c[k]
    assert all(v >= 100 for v in seen.values()), f"the mirror met too few collisions for the comparison to show much: {seen}"


@pytest.mark.parametrize("name", pc.GRIDS)
def test_every_count_of_points(name):
    """the tails of a wave and of a workgroup, n = 0 and n = 1 (points are independent: a prefix of the set gives a prefix of the result)"""
    o, vel, _, xyz = pc.case(name)
    u = pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX))
    check(rig(name), OracleGrid(o), u, cc.sdf_of(name, "full"), dev_sdf(name, "full"), xyz, pc.DT, 2, 3, "push", f"{name} counts", n_list=pc.COUNTS)


def test_optional_outputs_may_be_absent():
    name = "ragged32"
    o, vel, _, xyz = pc.case(name)
    R = rig(name)
    u = pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX))
    want, status, hit, _ = cc.collide_mirror(OracleGrid(o), u, cc.sdf_of(name, "full"), xyz, pc.DT, pc.INV_DX, 2, 2, "kill")
    for with_status, with_hit in ((False, False), (True, False), (False, True)):
        p = R.dev(xyz)
        st = R.t.full((len(xyz),), STATUS_SENTINEL, dtype=R.t.uint8, device="cuda") if with_status else None
        ht = R.t.full((len(xyz),), STATUS_SENTINEL, dtype=R.t.uint8, device="cuda") if with_hit else None
        R.D.trace_points_collide(R.grid, R.dev(u), dev_sdf(name, "full"), p, pc.DT, pc.INV_DX, 2, 2, mode="kill", status=st, hit=ht)
        assert_words(p.cpu().numpy(), want, "positions")
        assert st is None or np.array_equal(st.cpu().numpy(), status)
        assert ht is None or np.array_equal(ht.cpu().numpy(), hit)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_push_against_a_positive_sdf_is_the_plain_trace(order):
    """no sample is below the threshold: the positions are hns_dev_trace_points' word for word, status too, and hit is 0"""
    name = "ragged32"
    o, vel, _, xyz = pc.case(name)
    R = rig(name)
    u = R.dev(pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX)))
    positive = R.dev(np.abs(cc.sdf_of(name, "full")) + F(0.01))
    plain, plain_status = R.trace(u, xyz, pc.DT, pc.INV_DX, order, 3, "plain")
    got, status, hit = trace_collide(R, u, positive, xyz, pc.DT, pc.INV_DX, order, 3, "push", "positive sdf")
    assert_words(got, plain, f"order {order}: positions against hns_dev_trace_points")
    assert np.array_equal(status, plain_status) and not hit.any() and (got != xyz).any()


@pytest.mark.parametrize("name", ["one_leaf", "ragged32"])
def test_special_sdf_values_equal_the_device_semantics_mirror(name):
    """NaN, +-inf, -0.0 and subnormals planted in the SDF: a NaN sample is no collision, and every bit of the rest is the mirror's on the oracle's device build"""
    o, vel, _, xyz = pc.case(name)
    xyz = xyz[:257]
    R, D = rig(name), OracleGrid(o, lib=oracle_device())
    rng = np.random.default_rng([9, pc.GRIDS.index(name)])
    u = pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX))
    for cls in ("nonfinite", "subnormal", "zeros"):
        sdf = sc.plant(cls, cc.sdf_of(name, "full"), rng, rate=0.05)
        if cls == "nonfinite":
            assert np.isnan(sdf).any() and np.isposinf(sdf).any() and np.isneginf(sdf).any()
        for mode in cc.MODES:
            want, status, hit, _ = check(R, D, u, sdf, R.dev(sdf), xyz, pc.DT, 2, 2, mode, f"{name} {cls} {mode}", same=assert_same_bits)
            assert hit.any() and (hit == 0).any()


SIM_NAMES = ["density", "temperature", "fuel", "waste", "flame", "collision_sdf"]
SIM_VS = 1.0 / 32


def collide_sims(o, masks):
    state = random_state(11, len(o), SIM_NAMES)
    state["collision_sdf"] = np.array(cc.lattice_sdf(OracleGrid(o).coords()))
    pair = [make_sim(o, SIM_NAMES, state, masks, SIM_VS) for _ in range(2)]
    return pair[0][1], pair[1][1], [g for g, _ in pair]


def test_sim_calls_equal_the_device_calls_and_leave_the_sim_alone():
    o, _, _, xyz = pc.case("ragged32")
    s, twin, keep = collide_sims(o, random_masks(5, len(o)))
    for sim in (s, twin):
        for _ in range(2):  # (two core substeps with one dt: the second looks ahead, and its memo is pending while the points are traced)
            sim.core_substep(3, 0.04, SIM_VS)
    now = download(s, SIM_NAMES)
    R = Rig(o, now["vel"], [now["collision_sdf"]], SIM_VS)
    G = OracleGrid(o)
    inv_dx = float(F(1.0) / F(SIM_VS))
    dt = 0.04  # (velocities of order one at 32 voxels per unit: steps of a voxel or two)
    total = 0
    for mode, order, steps in (("stop", 2, 1), ("push", 4, 3), ("kill", 1, 2)):
        q = R.dev(xyz)
        st, ht = s.trace(q, dt=dt, voxel_size=SIM_VS, order=order, steps=steps, status=True, collide=mode, hit=True, **SPEC)
        wq, wst, wht = trace_collide(R, R.vel, R.phi[0], xyz, dt, inv_dx, order, steps, mode, "sim")
        assert_words(q.cpu().numpy(), wq, f"Sim.trace collide={mode}")
        assert np.array_equal(st.cpu().numpy(), wst) and np.array_equal(ht.cpu().numpy(), wht)
        want, status, hit, _ = cc.collide_mirror(G, now["vel"], now["collision_sdf"], xyz, dt, inv_dx, order, steps, mode)
        assert_words(wq, want, f"Sim.trace collide={mode} against the mirror")
        assert np.array_equal(wst, status) and np.array_equal(wht, hit)
        total += int((hit & 7 != 0).sum())
        only_status = s.trace(R.dev(xyz), dt=dt, voxel_size=SIM_VS, order=order, steps=steps, status=True, collide=mode, **SPEC)
        assert np.array_equal(only_status.cpu().numpy(), wst)
        assert s.trace(R.dev(xyz), dt=dt, voxel_size=SIM_VS, order=order, steps=steps, collide=mode, **SPEC) is None
    assert total >= 100, "almost no point of the sim met the collider"
    # the sim is as its twin, which traced nothing: fields, masks, what it looked ahead, and the next substep
    for k, v in download(twin, SIM_NAMES).items():
        assert_words(download(s, SIM_NAMES)[k], v, f"after the point calls: {k}")
    assert np.array_equal(s.active_masks(), twin.active_masks())
    assert s.lookahead_counts() == twin.lookahead_counts() and s.lookahead_counts()[0] >= 1
    for sim in (s, twin):
        sim.core_substep(3, 0.04, SIM_VS)
    assert s.lookahead_counts() == twin.lookahead_counts() and s.lookahead_counts()[1] >= 1, "the memo was not consumed as on the twin"
    after, after_twin = download(s, SIM_NAMES), download(twin, SIM_NAMES)
    for k in after:
        assert_words(after[k], after_twin[k], f"a substep after the point calls: {k}")
    s.close(), twin.close()
    del keep


def test_a_frame_step_drops_the_killed_points_on_the_device():
    """Sim.trace(collide="kill"), PointPopulation.select(status, 1), compact: the live count is the mirror's status.sum() and the rows are the mirror's survivors, in order"""
    from hnanosolver_amd import device

    o, vel, _, xyz = pc.case("ragged32")
    s, twin, keep = collide_sims(o, None)
    twin.close()
    state_vel = pc.scaled_velocity(vel, 4.0, F(0.04) * F(1.0 / SIM_VS))
    s.upload({"vel": np.ascontiguousarray(state_vel)})
    now = download(s, SIM_NAMES)
    inv_dx = float(F(1.0) / F(SIM_VS))
    want, status, hit, _ = cc.collide_mirror(OracleGrid(o), now["vel"], now["collision_sdf"], xyz, 0.04, inv_dx, 2, 3, "kill")
    assert (hit & cc.HIT_KILLED).astype(bool).sum() >= 50 and 400 <= status.sum() < len(xyz) - 50
    R = Rig(o, now["vel"], [])
    q = R.dev(xyz)
    st = s.trace(q, dt=0.04, voxel_size=SIM_VS, order=2, steps=3, status=True, collide="kill", **SPEC)
    pop = device.PointPopulation(keep[0], len(xyz))
    rows = pop.select(st, 1).compact(q, fill=float("nan"))
    live, wanted = pop.counts()
    assert live == wanted == int(status.sum())
    got = rows.cpu().numpy()
    assert_words(got[:live], want[status == 1], "the survivors' rows")
    assert np.isnan(got[live:]).all() and len(got) == len(xyz)
    pop.close(), s.close()
    del keep


def test_an_empty_grid_moves_nothing():
    import torch

    from hnanosolver_amd import api, device

    g = api.create_grid_from_leaves(np.zeros((0, 3), np.int32), 1.0 / 24)
    xyz = pc.case("one_leaf")[3][:65]
    p = torch.from_numpy(np.array(xyz)).cuda()
    st, ht = torch.full((65,), 7, dtype=torch.uint8, device="cuda"), torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    device.trace_points_collide(g, torch.zeros((1, 3), device="cuda"), torch.zeros(1, device="cuda"), p, 0.04, 24.0, 2, 2, mode="push", status=st, hit=ht)
    assert_words(p.cpu().numpy(), xyz, "an empty grid")
    assert not st.cpu().numpy().any() and not ht.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------
# late, on a non-blocking stream, inside guard bands (tests/stream_cases.py; as tests/test_streams_gpu.py holds hns_dev_trace_points)
# ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def stream_ctx(grid):
    import stream_cases

    return stream_cases.Ctx(grid)


@pytest.mark.parametrize("name", ["hns_dev_trace_points_collide", "hns_sim_trace_points_collide"])
def test_entry_point_late_on_a_non_blocking_stream(name):
    import stream_cases
    import torch

    entry = stream_cases.CASES[name]
    delay = stream_cases.Delay(torch)
    for grid in entry.grids:
        x = stream_ctx(grid)
        case = entry.variants[stream_cases.COLLIDE_VARIANT](x)
        what = f"{name}[{stream_cases.COLLIDE_VARIANT}-{grid}]"
        if entry.level == "kernel":
            stream_cases.check_call(torch, case, delay, what)
        else:
            stream_cases.check_sim_case(torch, x, case, delay, what)
