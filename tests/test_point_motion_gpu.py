"""Points with a velocity of their own on the GPU: hns_point_motion_* (k_move_points of hns_point_motion.hip) through device.PointMotion and Sim.point_motion, against the
numpy mirror of tests/point_motion_cases.py, which restates include/hns.h on the oracle's samplers.

There is no tolerance anywhere: positions, velocities and ages are compared as 32-bit words, status and hit as bytes; a NaN counts as equal to any NaN only in the
special-value test, as in tests/test_points_collide_gpu.py. The sim holds the grid's velocity and its collision SDF at the voxel size of
tests/test_points_collide_gpu.py (1 / 32: inv_dx = 32). The conditions the inputs meet -- how many points start inside, bounce, are reflected, need a later push, are put
back, expire -- are held without a GPU by tests/test_point_motion_cases.py."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import point_motion_cases as mc
import points_cases as pc
import points_collide_cases as cc
import special_cases as sc
from frame_cases import download, make_sim, random_masks
from hnanosolver_amd import _lib
from oracle_lib import OracleGrid, oracle_device
from test_points_collide_gpu import SIM_VS
from test_points_gpu import assert_same_bits, assert_words

pytestmark = pytest.mark.gpu

F = np.float32
INV_DX = float(F(1.0) / F(SIM_VS))
NAMES = ["density", "collision_sdf"]
GRIDS = ("ragged32", "sparse_far", "one_leaf")  # 32, 22 and 1 leaves
ARRAYS = ("xyz", "vel", "age", "status", "hit")
WORD, BYTE = 0xDEADBEEF, 0xAB  # what the rows hold before they are filled


def state_of(name, variant="full", sdf=None, vel=None):
    o, v, phi, _ = pc.case(name)
    return {"vel": np.array(v if vel is None else vel), "density": np.array(phi[0]), "collision_sdf": np.array(cc.sdf_of(name, variant) if sdf is None else sdf)}


@functools.lru_cache(maxsize=None)
def _sim(name):
    return make_sim(pc.case(name)[0], NAMES, state_of(name), None, SIM_VS)


def sim_of(name, sdf=None):
    """(grid, sim) of a grid of points_cases.GRIDS, made once, holding the grid's velocity and `sdf` (None: the full lattice SDF) as collision_sdf"""
    g, s = _sim(name)
    s.upload({"collision_sdf": np.array(cc.sdf_of(name, "full") if sdf is None else sdf, dtype=F)})
    return g, s


def plant(motion):
    """every row of every array holds the sentinel"""
    import torch

    for k in ("xyz", "vel", "age"):
        getattr(motion, k).view(torch.int32).fill_(WORD - (1 << 32))
    motion.status.fill_(BYTE), motion.hit.fill_(BYTE)


def fill(motion, xyz, v, age):
    import torch

    n = len(xyz)
    if n:
        motion.xyz[:n] = torch.from_numpy(np.array(xyz, dtype=F)).cuda()
        motion.vel[:n] = torch.from_numpy(np.array(v, dtype=F)).cuda()
        motion.age[:n] = torch.from_numpy(np.array(age, dtype=F)).cuda()


def read(motion, n=None):
    """the five arrays as numpy copies (their first n rows)"""
    return tuple(getattr(motion, k)[: motion.capacity if n is None else n].cpu().numpy() for k in ARRAYS)


def assert_equal(got, want, what, same=assert_words):
    for k, g, w in zip(ARRAYS[:3], got, want):
        same(g, w, f"{what}: {k}")
    for k, g, w in zip(ARRAYS[3:], got[3:], want[3:]):
        bad = np.flatnonzero(g != w)
        assert not len(bad), f"{what}: {k} differs at {bad[:6].tolist()}: {g[bad[:6]]} vs {w[bad[:6]]}"


# ---------------------------------------------------------------------------------------------------------------
# 1. the mirror
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("name", GRIDS)
def test_steps_equal_the_mirror(name, mode):
    """the full 4,099 points over both SDF variants, both signs of dt, 1 and 3 steps"""
    o, vel, _, xyz = pc.case(name)
    v, age = mc.inputs(name)
    g, s = sim_of(name)
    G = OracleGrid(o)
    seen = 0
    with s.point_motion(len(xyz)) as m:
        for variant in cc.VARIANTS:
            sdf = cc.sdf_of(name, variant)
            s.upload({"collision_sdf": np.array(sdf)})
            for dt in (mc.DT, -mc.DT):
                for steps in (1, 3):
                    want = mc.motion_mirror(G, vel, None if mode == "free" else sdf, xyz, v, age, dt, INV_DX, steps, mode, {})
                    fill(m, xyz, v, age)
                    m.step(s, len(xyz), dt, SIM_VS, steps, mode, **mc.SPEC)
                    assert_equal(read(m), want, f"{name} {variant} {mode} dt {dt} steps {steps}")
                    seen += int((want[4] & 7 != 0).sum())
                    assert want[3].any() and not want[3].all()
    assert mode == "free" or seen >= 1000, f"the mirror met too few collisions for the comparison to show much: {seen}"


# ---------------------------------------------------------------------------------------------------------------
# 2. row counts, and where the arrays lie
# ---------------------------------------------------------------------------------------------------------------


def test_every_count_of_rows_and_the_rows_beyond_keep_their_bytes():
    name = "ragged32"
    o, vel, _, xyz = pc.case(name)
    v, age = mc.inputs(name)
    g, s = sim_of(name)
    want = mc.expected(name, "full", "bounce", mc.DT, mc.STEPS, INV_DX)
    cap = len(xyz) + 64
    with s.point_motion(cap) as m:
        assert m.capacity == cap and tuple(m.xyz.shape) == (cap, 3) and tuple(m.vel.shape) == (cap, 3) and tuple(m.age.shape) == tuple(m.status.shape) == tuple(m.hit.shape) == (cap,)
        for n in (0, 1, 63, 64, 65, 255, 256, 257, len(xyz)):
            plant(m)
            fill(m, xyz[:n], v[:n], age[:n])
            m.step(s, n, mc.DT, SIM_VS, mc.STEPS, "bounce", **mc.SPEC)
            got = read(m)
            assert_equal([a[:n] for a in got], [a[:n] for a in want[:5]], f"n = {n}")
            for k, a in zip(ARRAYS, got):
                rest = a[n:]
                assert (rest.view(np.uint32) == WORD).all() if rest.dtype == F else (rest == BYTE).all(), f"n = {n}: {k} was written behind row n - 1"
        # the arrays of get: disjoint, each behind the one before at the pool's 256-byte slices -- one block
        info = _lib.hns_point_motion_info()
        assert _lib.lib.hns_point_motion_get(m._ptr, C.byref(info)) == 0 and info.capacity == cap
        at = [info.xyz, info.vel, info.age, info.status, info.hit]
        size = [12 * cap, 12 * cap, 4 * cap, cap, cap]
        assert all(a and a % 256 == 0 for a in at)
        for i in range(4):
            assert at[i + 1] == at[i] + (size[i] + 255) // 256 * 256, "the five arrays are not consecutive slices of one block"
        assert [t.data_ptr() for t in (m.xyz, m.vel, m.age, m.status, m.hit)] == at
        with pytest.raises(ValueError, match="capacity"):
            m.step(s, cap + 1, mc.DT, SIM_VS)


# ---------------------------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["one_leaf", "ragged32"])
def test_special_values_equal_the_device_semantics_mirror(name):
    """NaN, +-inf, -0.0 and subnormals planted in the point velocities, the ages and the SDF, NaN and inf in some positions: every bit is the mirror's on the oracle's device
    build, a NaN equal to any NaN; a row without a position keeps every bit"""
    o, vel, _, xyz = pc.case(name)
    v0, age0 = mc.inputs(name)
    n = 513
    g, s = sim_of(name)
    D = OracleGrid(o, lib=oracle_device())
    rng = np.random.default_rng([13, pc.GRIDS.index(name)])
    x = np.array(xyz[:n])
    x[5::16, 0] = np.nan
    x[6::32, 1] = np.inf
    x[7::32, 2] = -np.inf
    gone = ~np.isfinite(x).all(1)
    with s.point_motion(n) as m:
        for cls in ("nonfinite", "subnormal", "zeros"):
            sdf = sc.plant(cls, cc.sdf_of(name, "full"), rng, rate=0.05)
            v, age = sc.plant(cls, v0[:n], rng, rate=0.05), sc.plant(cls, age0[:n], rng, rate=0.05)
            if cls == "nonfinite":
                assert np.isnan(sdf).any() and np.isposinf(sdf).any() and np.isneginf(sdf).any() and np.isnan(v).any() and np.isinf(v).any() and np.isnan(age).any()
            s.upload({"collision_sdf": sdf})
            for mode in mc.MODES:
                want = mc.motion_mirror(D, vel, None if mode == "free" else sdf, x, v, age, mc.DT, INV_DX, 2, mode, {})
                plant(m)
                fill(m, x, v, age)
                m.step(s, n, mc.DT, SIM_VS, 2, mode, **mc.SPEC)
                got = read(m)
                assert_equal(got, want, f"{name} {cls} {mode}", same=assert_same_bits)
                for k, a, b in zip(ARRAYS[:3], got, (x, v, age)):
                    assert_words(a[gone], b[gone], f"{name} {cls} {mode}: {k} of a row without a position")
                assert not got[3][gone].any() and not got[4][gone].any()
                assert mode == "free" or (want[4].any() and (want[4] == 0).any())


# ---------------------------------------------------------------------------------------------------------------
# 4. mode free
# ---------------------------------------------------------------------------------------------------------------


def test_free_needs_no_collision_sdf_and_a_positive_sdf_is_free():
    name = "ragged32"
    o, vel, phi, xyz = pc.case(name)
    v, age = mc.inputs(name)
    n = len(xyz)
    want = mc.expected(name, "full", "free", mc.DT, mc.STEPS, INV_DX)
    g0, bare = make_sim(o, ["density"], {"vel": np.array(vel), "density": np.array(phi[0])}, None, SIM_VS)
    with bare.point_motion(n) as m:
        fill(m, xyz, v, age)
        m.step(bare, n, mc.DT, SIM_VS, mc.STEPS, "free", **mc.SPEC)
        free = read(m)
        assert_equal(free, want, "free on a sim without collision_sdf")
        assert not free[4].any() and (free[0] != xyz).any()
        for mode in ("stick", "bounce", "kill"):
            with pytest.raises(ValueError, match="collision_sdf"):  # (HNS_ERR_INVALID_ARGUMENT surfaces as ValueError)
                m.step(bare, n, mc.DT, SIM_VS, mc.STEPS, mode, **mc.SPEC)
        with pytest.raises(ValueError, match="bogus"):
            m.step(bare, n, mc.DT, SIM_VS, mode="bogus")
        assert_equal(read(m), free, "after the refusals")
    bare.close()
    g, s = sim_of(name, np.abs(cc.sdf_of(name, "full")) + F(0.01))
    with s.point_motion(n) as m:
        fill(m, xyz, v, age)
        m.step(s, n, mc.DT, SIM_VS, mc.STEPS, "bounce", **mc.SPEC)
        got = read(m)
        assert_equal(got[:3], free[:3], "bounce against a positive SDF")
        assert np.array_equal(got[3], free[3]) and not got[4].any()


# ---------------------------------------------------------------------------------------------------------------
# 5. late, on a non-blocking stream
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fill_byte", [None, 255])
def test_step_late_on_a_non_blocking_stream(fill_byte):
    """xyz, vel, age and the sim's fields arrive behind a delay on a non-blocking stream (until then they hold NaN): the result is the null-stream run's and the mirror's.
    With arena_fill 255 around create the object's block holds 0xFF when it is handed out."""
    import torch

    import stream_cases
    from pool_cases import arena_fill
    from hnanosolver_amd import api, device

    name = "ragged32"
    o, vel, phi, xyz = pc.case(name)
    v, age = mc.inputs(name)
    n = len(xyz)
    want = mc.expected(name, "full", "bounce", mc.DT, mc.STEPS, INV_DX)
    grid = api.create_grid_from_leaves(o, SIM_VS)
    sim = device.Sim(grid, NAMES)
    N = len(o) * 512
    nan = {"vel": np.full((N, 3), stream_cases.NAN_WORD, np.uint32).view(F), **{k: np.full(N, stream_cases.NAN_WORD, np.uint32).view(F) for k in NAMES}}
    keep = {k: torch.from_numpy(a).pin_memory() for k, a in state_of(name).items()}  # pinned: hns_sim_upload's copies are asynchronous
    state = {k: t.numpy() for k, t in keep.items()}
    if fill_byte is None:
        m = sim.point_motion(n)
    else:
        with arena_fill(fill_byte):
            m = sim.point_motion(n)
        torch.cuda.synchronize()
        assert (m.status.cpu().numpy() == fill_byte).all() and (m.xyz.view(torch.int32).cpu().numpy() == -1).all()
    try:
        dev = lambda a: torch.from_numpy(np.array(a, dtype=F)).cuda()
        tensors = {k: getattr(m, k) for k in ARRAYS}
        operands = {k: stream_cases.Operand(tensors[k], dev(a)) for k, a in (("xyz", xyz), ("vel", v), ("age", age))}

        def fn(stream):
            sim.upload(state, stream)
            m.step(sim, n, mc.DT, SIM_VS, mc.STEPS, "bounce", stream=stream, **mc.SPEC)

        # the null stream, the device idle before and after
        sim.upload(nan)
        for op in operands.values():
            op.arrive()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(0)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        ref = read(m)
        assert_equal(ref, want, "the null-stream run against the mirror")
        # late
        sim.upload(nan)
        delay = stream_cases.Delay(torch)
        rec = stream_cases.late_call(fn, operands, tensors, delay, delay.for_host_time(host), True, None, "PointMotion.step")
        assert_equal([rec.outputs[k].cpu().numpy() for k in ARRAYS], ref, "late on a non-blocking stream")
    finally:
        torch.cuda.synchronize()
        m.close(), sim.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. the sim is only read, and a regrid is followed
# ---------------------------------------------------------------------------------------------------------------


def test_the_sim_is_only_read_and_a_regrid_is_followed():
    name = "ragged32"
    o, vel, _, xyz = pc.case(name)
    v, age = mc.inputs(name)
    n = len(xyz)
    masks = random_masks(5, len(o))
    (g1, s), (g2, twin) = (make_sim(o, NAMES, state_of(name), masks, SIM_VS) for _ in range(2))
    for sim in (s, twin):
        for _ in range(2):  # (two core substeps with one dt: the second looks ahead, and its memo is pending while the points are stepped)
            sim.core_substep(3, 0.04, SIM_VS)
    now = download(s, NAMES)
    m = s.point_motion(n)
    fill(m, xyz, v, age)
    for mode in mc.MODES:
        m.step(s, n, mc.DT, SIM_VS, 1, mode, **mc.SPEC)
    want = (xyz, v, age)
    for mode in mc.MODES:
        want = mc.motion_mirror(OracleGrid(o), now["vel"], now["collision_sdf"], *want[:3], mc.DT, INV_DX, 1, mode, {})
    assert_equal(read(m), want, "four steps on the sim's current fields")
    # the sim is as its twin, which stepped nothing: fields, masks, what it looked ahead, and the next substep
    for k, a in download(twin, NAMES).items():
        assert_words(download(s, NAMES)[k], a, f"after the steps: {k}")
    assert np.array_equal(s.active_masks(), twin.active_masks())
    assert s.lookahead_counts() == twin.lookahead_counts() and s.lookahead_counts()[0] >= 1
    for sim in (s, twin):
        sim.core_substep(3, 0.04, SIM_VS)
    assert s.lookahead_counts() == twin.lookahead_counts() and s.lookahead_counts()[1] >= 1, "the memo was not consumed as on the twin"
    after, after_twin = download(s, NAMES), download(twin, NAMES)
    for k in after:
        assert_words(after[k], after_twin[k], f"a substep after the steps: {k}")
    # a regrid between two steps: the same object, the new grid
    before = read(m)
    keep = s.regrid(1)
    o2 = np.ascontiguousarray(s.grid.coords()[::512], dtype=np.int32)
    assert len(o2) != len(o) or (o2 != o).any()
    now2 = download(s, NAMES)
    G2 = OracleGrid(o2)
    assert (pc.taps_inside(OracleGrid(o), before[0]) != pc.taps_inside(G2, before[0])).mean() > 0.05  # (points the old grid answers differently)
    m.step(s, n, mc.DT, SIM_VS, 2, "bounce", **mc.SPEC)
    want2 = mc.motion_mirror(G2, now2["vel"], now2["collision_sdf"], *before[:3], mc.DT, INV_DX, 2, "bounce", {})
    assert_equal(read(m), want2, "after a regrid")
    del keep
    m.close(), s.close(), twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the frame loop
# ---------------------------------------------------------------------------------------------------------------


def test_a_frame_step_drops_the_dead_the_escaped_and_the_expired_on_the_device():
    """step(kill, max_age), PointPopulation.select(motion.status, 1), compact of xyz, vel and age: the live count is the mirror's status.sum() and the rows are the mirror's
    survivors, in order"""
    import torch

    name = "ragged32"
    o, vel, _, xyz = pc.case(name)
    n = len(xyz)
    g, s = sim_of(name)
    x, v, age, status, hit, _ = mc.expected(name, "full", "kill", mc.DT, mc.STEPS, INV_DX)
    expired = np.isfinite(x).all(1) & ~(age < F(mc.SPEC["max_age"]))
    assert ((hit & mc.HIT_KILLED) != 0).sum() >= 50 and expired.sum() >= 50 and 400 <= status.sum() < n - 100
    with s.point_motion(n) as m:
        fill(m, xyz, *mc.inputs(name))
        m.step(s, n, mc.DT, SIM_VS, mc.STEPS, "kill", **mc.SPEC)
        pop = s.point_population(n)
        pop.select(m.status, 1)
        rows = [pop.compact(src, fill=float("nan")) for src in (m.xyz, m.vel, m.age.reshape(n, 1))]
        live, wanted = pop.counts()
        assert live == wanted == int(status.sum())
        for k, got, w in zip(ARRAYS, rows, (x, v, age.reshape(n, 1))):
            got = got.cpu().numpy()
            assert_words(got[:live], w[status == 1], f"the survivors' rows of {k}")
            assert np.isnan(got[live:]).all() and len(got) == n
        pop.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# 8. a grid without leaves
# ---------------------------------------------------------------------------------------------------------------


def test_on_a_grid_without_leaves_points_still_fall():
    """U = 0 and S = 0, no leaf exists: the rows fall under gravity and every status is 0"""
    from hnanosolver_amd import api, device

    g = api.create_grid_from_leaves(np.zeros((0, 3), np.int32), SIM_VS)
    s = device.Sim(g, ["collision_sdf"])
    xyz = pc.case("one_leaf")[3][:65]
    v, age = (a[:65] for a in mc.inputs("one_leaf"))
    with s.point_motion(65) as m:
        for mode in mc.MODES:
            plant(m)
            fill(m, xyz, v, age)
            m.step(s, 65, mc.DT, SIM_VS, 2, mode, **mc.SPEC)
            want = mc.motion_mirror(None, None, None, xyz, v, age, mc.DT, INV_DX, 2, mode, {})
            assert_equal(read(m), want, f"no leaves, {mode}")
            assert not want[3].any() and not want[4].any() and (want[1] != v).any()
    s.close()
