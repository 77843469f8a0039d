"""Fields sampled at points and points traced through the velocity on the GPU: hns_dev_sample_points / hns_dev_trace_points (k_sample_points, k_trace_points of
hns_points.hip), the two calls on a sim's own buffers and their Python mirrors.

Every comparison is equality of 32-bit words (status: of bytes): float samples against the oracle and the reference's own sampler build, Vec3f samples against the oracle on
the fmaf branch of its lerp, traced positions against the mirror of tests/points_cases.py. A NaN counts as equal to any NaN only in the special-value tests, as in
tests/test_special_values_gpu.py: the sign of a NaN an operation makes is the instruction set's, and x86 and gfx950 differ in it. The point sets and the conditions they
meet (counted by the oracle) are tests/points_cases.py's; tests/test_points_cases.py holds them without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import points_cases as pc
import special_cases as sc
from frame_cases import LAUNCH_RANGES, download, launch_range, make_sim, random_state
from oracle_lib import OracleGrid, oracle_device, reference_samplers

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 24.0
SENTINEL = np.frombuffer(np.uint32(0xDEADBEEF).tobytes(), F)[0]  # what an output holds before a call
STATUS_SENTINEL = 0xAB


def words(a):
    return np.ascontiguousarray(a, dtype=F).reshape(-1).view(np.uint32)


def assert_words(got, want, what):
    """equal as 32-bit words: zero signs, subnormals, inf, and the sign and payload of every NaN"""
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    d = np.flatnonzero(g != w)
    assert len(d) == 0, f"{what}: {len(d)} of {g.size} words differ; first at {d[:6].tolist()}: {[hex(x) for x in g[d[:6]]]} vs {[hex(x) for x in w[d[:6]]]}"


def assert_same_bits(got, want, what):
    """as assert_words, a NaN equal to any NaN (special_cases.same_bits)"""
    assert np.asarray(got).shape == np.asarray(want).shape, what
    assert sc.same_bits(got, want), f"{what}: {sc.describe(got, want)}"


class Rig:
    """a device grid over a leaf set with device copies of its fields; outputs are made one element longer than asked and start as SENTINEL"""

    def __init__(self, origins, vel, phi, vs=VS):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.o = np.ascontiguousarray(origins, dtype=np.int32)
        self.grid = api.create_grid_from_leaves(self.o, vs)
        self.vel, self.phi = self.dev(vel), [self.dev(p) for p in phi]

    def dev(self, a):
        return self.t.from_numpy(np.array(a, dtype=F)).cuda()

    def points(self, xyz):
        """(device tensor of len(xyz) + 1 rows, its first len(xyz) rows): no call ever gets a null pointer for n = 0, and the row behind the last is watched"""
        full = self.t.full((len(xyz) + 1, 3), float(SENTINEL), dtype=self.t.float32, device="cuda")
        full[: len(xyz)] = self.dev(np.asarray(xyz, dtype=F).reshape(-1, 3))
        return full, full[: len(xyz)]

    def sample(self, fields, xyz, what=""):
        """-> outputs (numpy, n rows each) of one hns_dev_sample_points call over `fields`; asserts that the element behind the last kept the sentinel and xyz its words"""
        n = len(xyz)
        pfull, p = self.points(xyz)
        full = [self.t.full((n + 1, 3) if f.dim() == 2 else (n + 1,), float(SENTINEL), dtype=self.t.float32, device="cuda") for f in fields]
        self.D.sample_points(self.grid, fields, p, [f[:n] for f in full])
        got = [f.cpu().numpy() for f in full]
        for i, g in enumerate(got):
            assert (words(g[n:]) == 0xDEADBEEF).all(), f"{what}: output {i} was written behind its last element"
        assert_words(pfull.cpu().numpy()[:n], xyz, f"{what}: xyz")
        return [g[:n] for g in got]

    def trace(self, vel, xyz, dt, inv_dx, order, steps, what=""):
        """-> (positions, status) of one hns_dev_trace_points call; the row and the byte behind the last are watched"""
        n = len(xyz)
        pfull, p = self.points(xyz)
        st = self.t.full((n + 1,), STATUS_SENTINEL, dtype=self.t.uint8, device="cuda")
        self.D.trace_points(self.grid, vel, p, dt, inv_dx, order, steps, st[:n])
        got, status = pfull.cpu().numpy(), st.cpu().numpy()
        assert (words(got[n:]) == 0xDEADBEEF).all() and status[n] == STATUS_SENTINEL, f"{what}: written behind the last point"
        return got[:n], status[:n]


@functools.lru_cache(maxsize=None)
def rig(name):
    o, vel, phi, _ = pc.case(name)
    return Rig(o, vel, phi)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's samples of the eleven float fields and of the velocity (fmaf branch) at the grid's 4,099 points: computed once"""
    o, vel, phi, xyz = pc.case(name)
    G = OracleGrid(o)
    if name != "one_leaf":
        pc.check_conditions(G, xyz, name)
    want_f = [G.sample_trilinear_f(p, xyz) for p in phi]
    with pc.fma_branch():
        want_v = G.sample_trilinear_v(vel, xyz)
    return want_f, want_v


def mixed_fields(R):
    """(thirteen fields in mixed ncomp, the velocity third and twelfth; which float field each entry is, -1 = the velocity)"""
    which = [0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, -1, 10]
    return [R.vel if k < 0 else R.phi[k] for k in which], which


# ---------------------------------------------------------------------------------------------------------------
# 1. sampling
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", pc.COUNTS)
@pytest.mark.parametrize("name", pc.GRIDS)
def test_samples_equal_the_oracle(name, n):
    R, (want_f, want_v) = rig(name), expected(name)
    xyz = pc.case(name)[3][:n]
    fields, which = mixed_fields(R)
    got = R.sample(fields, xyz, f"{name} n={n}")  # thirteen fields: a launch of eight and one of five
    assert len(got) == len(which)
    for i, k in enumerate(which):
        want = want_v[:n] if k < 0 else want_f[k][:n]
        assert got[i].shape == want.shape
        assert (words(got[i]) != 0xDEADBEEF).all() or n == 0, f"{name} n={n}: output {i} kept a sentinel"
        assert_words(got[i], want, f"{name} n={n}: output {i} (field {k})")


@pytest.mark.parametrize("name", pc.GRIDS)
def test_float_samples_equal_the_reference_build(name):
    Rf = reference_samplers()
    if Rf is None:
        pytest.skip("oracle/_ref/libhns_ref.so not available (needs the reference checkout to build)")
    o, _, phi, xyz = pc.case(name)
    g = Rf.ref_grid_create(o.ctypes.data, len(o))
    try:
        order = np.zeros((len(o), 3), np.int32)
        Rf.ref_leaf_origins(g, order.ctypes.data)
        assert np.array_equal(order, o), "the leaf set is not in the reference's leaf order: its flat arrays would differ"
        R = rig(name)
        got = R.sample(R.phi[:3], xyz, name)
        for i in range(3):
            want = np.zeros(len(xyz), F)
            Rf.ref_sample_trilinear_f(g, np.ascontiguousarray(phi[i]).ctypes.data, xyz.ctypes.data, len(xyz), want.ctypes.data)
            assert_words(got[i], want, f"{name}: field {i} against ref_sample_trilinear_f")
    finally:
        Rf.ref_grid_destroy(g)


@pytest.mark.parametrize("name", pc.GRIDS)
def test_many_field_calls_equal_one_field_calls(name):
    R = rig(name)
    xyz = pc.case(name)[3]
    fields, which = mixed_fields(R)
    alone = {k: R.sample([R.vel if k < 0 else R.phi[k]], xyz, f"{name} alone {k}")[0] for k in sorted(set(which))}
    for S in (1, 2, 8, 9, 11):  # both sides of the split at eight fields per launch
        got = R.sample(fields[:S], xyz, f"{name} S={S}")
        assert len(got) == S
        for i in range(S):
            assert_words(got[i], alone[which[i]], f"{name} S={S}: output {i}")


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_samples_and_traces_count_every_leaf_whatever_the_launch_range(kind):
    """include/hns.h: a leaf counts as inside whatever the grid's launch range, ghost leaves included -- the bytes of the whole range (which the tests around this one hold
    to the oracle and the mirror) under set_active_range on a strict inner range and under set_active_leaves(n // 2)"""
    name = "ragged32"
    R, (want_f, want_v) = rig(name), expected(name)
    o, vel, _, xyz = pc.case(name)
    fields, which = mixed_fields(R)
    u = R.dev(pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX)))
    whole = R.sample(fields, xyz, "whole range")
    whole_xyz, whole_status = R.trace(u, xyz, pc.DT, pc.INV_DX, 2, 3, "whole range")
    assert 0 < whole_status.sum() < len(xyz)
    with launch_range(R.grid, kind):
        got = R.sample(fields, xyz, kind)
        got_xyz, got_status = R.trace(u, xyz, pc.DT, pc.INV_DX, 2, 3, kind)
    assert R.grid.active_leaves() == len(o)
    for i, k in enumerate(which):
        assert_words(got[i], whole[i], f"{kind}: output {i} (field {k}) against the whole range")
        assert_words(got[i], want_v if k < 0 else want_f[k], f"{kind}: output {i} (field {k}) against the oracle")
    assert_words(got_xyz, whole_xyz, f"{kind}: traced positions")
    assert np.array_equal(got_status, whole_status), f"{kind}: status"


# ---------------------------------------------------------------------------------------------------------------
# 2. tracing
# ---------------------------------------------------------------------------------------------------------------


def check_trace(R, G, vel_np, xyz, dt, inv_dx, order, steps, what, same=assert_words, n_list=None):
    path, status = pc.trace_mirror(G, vel_np, xyz, dt, inv_dx, order, steps)
    u = R.dev(vel_np)
    for n in n_list or (len(xyz),):
        got, st = R.trace(u, xyz[:n], dt, inv_dx, order, steps, what)
        same(got, path[-1][:n], f"{what} n={n}: positions")
        assert np.array_equal(st, status[:n]), f"{what} n={n}: status differs at {np.flatnonzero(st != status[:n])[:6].tolist()}"
    return path, status


@pytest.mark.parametrize("speed", pc.SPEEDS)
@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("name", pc.GRIDS)
def test_traces_equal_the_mirror(name, order, speed):
    o, vel, _, xyz = pc.case(name)
    R, G = rig(name), OracleGrid(o)
    moved = inside = 0
    for dt in (pc.DT, -pc.DT):
        u = pc.scaled_velocity(vel, speed, F(dt) * F(pc.INV_DX))
        for steps in (1, 3):
            tails = (len(xyz), 65, 1) if (steps == 1 and dt > 0) else None  # (points are independent: a prefix of the set gives a prefix of the result)
            path, status = check_trace(R, G, u, xyz, dt, pc.INV_DX, order, steps, f"{name} order {order} speed {speed} dt {dt} steps {steps}", n_list=tails)
            moved += int((path[-1] != path[0]).any(1).sum())
            inside += int(status.sum())
    assert moved >= 400 and inside >= 400, "the mirror moved almost nothing, or left almost nothing inside: the comparison would show little"


@pytest.mark.parametrize("order", [1, 4])
@pytest.mark.parametrize("name", ["sparse_far", "ragged32"])
def test_long_traces_beyond_the_cursors_reach(name, order):
    """eight steps of about 30 voxels: the leaf a thread found last is seldom a neighbour of the next cell's, and the lookup must go back to the origin hash"""
    o, vel, _, xyz = pc.case(name)
    u = pc.scaled_velocity(vel, 30.0, F(pc.DT) * F(pc.INV_DX))
    path, _ = check_trace(rig(name), OracleGrid(o), u, xyz, pc.DT, pc.INV_DX, order, 8, f"{name} order {order} steps 8")
    hop = np.abs(np.floor(path[1:] / 8.0) - np.floor(path[:-1] / 8.0)).max(2)  # leaves between consecutive positions, per step and point
    assert (hop >= 2).sum() >= 250 and ((hop >= 1) & (hop < 2)).sum() >= 1500, "steps beyond the neighbour leaves, and steps into them"


# ---------------------------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------------------------

SPECIALS = [sc.QNAN[0], sc.QNAN[1], F(np.inf), F(-np.inf), F(0.0), F(-0.0), F(1e-40), F(-1e-40), sc.SUB_MAX, -sc.SUB_MAX, F(3e9), F(-3e9)]
OUTSIDE_SPECIALS = 4  # NaN, -NaN, inf, -inf ... and, by index below, +-3e9: positions that are not finite or lie past int32


def special_points(o, seed):
    """(points, rows that carry a non-finite or a past-int32 coordinate, rows that carry a NaN): every special value on each axis of an inside position and on all three,
    among ordinary points"""
    rng = np.random.default_rng([seed, 7])
    rows, bad, nan = [], [], []
    for k, sv in enumerate(SPECIALS):
        for axes in ([0], [1], [2], [0, 1, 2]):
            p = (o[rng.integers(0, len(o))] + rng.uniform(0.0, 6.99, 3)).astype(F)
            p[axes] = sv
            rows.append(p)
            bad.append(k < OUTSIDE_SPECIALS or k >= len(SPECIALS) - 2)
            nan.append(k < 2)
    ordinary = pc.make_points(o, seed + 100, 200 - len(rows))
    xyz = np.concatenate([np.array(rows, dtype=F), ordinary]).astype(F)
    pad = np.zeros(len(ordinary), dtype=bool)
    return xyz, np.concatenate([np.array(bad), pad]), np.concatenate([np.array(nan), pad])


@pytest.mark.parametrize("name", pc.GRIDS)
def test_special_positions_equal_the_device_semantics_oracle(name):
    o, vel, phi, _ = pc.case(name)
    R, D = rig(name), OracleGrid(o, lib=oracle_device())
    xyz, bad, nan = special_points(o, pc.GRIDS.index(name))
    with pc.fma_branch(oracle_device()):
        want = [D.sample_trilinear_f(phi[0], xyz), D.sample_trilinear_f(phi[1], xyz), D.sample_trilinear_v(vel, xyz)]
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and (want[0][~bad] != 0).any()  # (the comparator shows NaN, finite values and non-zero ones)
    got = R.sample([R.phi[0], R.phi[1], R.vel], xyz, name)
    for i in range(3):
        assert_same_bits(got[i], want[i], f"{name}: special positions, output {i}")
    if name == "ragged32_off_origin":
        # A NaN coordinate converts to cell 0, and no leaf of this set is near it: by the oracle every tap of those cells is outside and reads 0. What the sampler
        # returns there is 0 + NaN * (0 - 0) = NaN -- the fraction is NaN - 0 -- in the reference's arithmetic, the oracle's and the kernel's alike.
        allnan = nan & np.isnan(xyz).all(1)
        assert allnan.sum() == 2 and (pc.taps_inside(D, xyz[allnan]) == 0).all()
        assert np.isnan(want[0][allnan]).all() and np.isnan(got[0][allnan]).all() and np.isnan(got[2][allnan]).all()
    # traced: such a point ends with status 0, and positions and status are the mirror's on the same oracle build
    u = pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX))
    for order in (1, 2, 4):
        path, status = check_trace(R, D, u, xyz, pc.DT, pc.INV_DX, order, 2, f"{name}: special positions, order {order}", same=assert_same_bits)
        assert (status[bad] == 0).all() and status[~bad].any()
        if name == "ragged32_off_origin":
            assert (status[: len(SPECIALS) * 4] == 0).all()  # (zeros and subnormals lie in cell 0 or -1: outside this set)


@pytest.mark.parametrize("name", ["ragged32", "sparse_far"])
def test_special_field_values_equal_the_device_semantics_oracle(name):
    o, vel, phi, xyz = pc.case(name)
    rng = np.random.default_rng([5, pc.GRIDS.index(name)])
    D = OracleGrid(o, lib=oracle_device())
    for cls in ("nonfinite", "subnormal", "zeros"):
        f, v = sc.plant(cls, phi[0], rng, rate=0.02), sc.plant(cls, vel, rng, rate=0.02)
        with pc.fma_branch(oracle_device()):
            want = [D.sample_trilinear_f(f, xyz), D.sample_trilinear_v(v, xyz)]
        if cls == "nonfinite":
            assert all(np.isnan(w).any() and np.isinf(w).any() and np.isfinite(w).mean() > 0.3 for w in want)
        if cls == "subnormal":
            assert all(sc.is_subnormal(w).any() for w in want)
        R = rig(name)
        got = R.sample([R.dev(f), R.dev(v)], xyz, f"{name} {cls}")
        for i in range(2):
            assert_same_bits(got[i], want[i], f"{name}: {cls} field values, output {i}")


# ---------------------------------------------------------------------------------------------------------------
# 4. on a sim
# ---------------------------------------------------------------------------------------------------------------

SIM_NAMES = ["density", "temperature", "fuel", "waste", "flame"]
SIM_VS = 1.0 / 32


def test_sim_calls_equal_the_device_calls_and_leave_the_sim_alone():
    o, _, _, xyz = pc.case("ragged32")
    state = random_state(11, len(o), SIM_NAMES)
    (g, s), (g2, twin) = make_sim(o, SIM_NAMES, state, None, SIM_VS), make_sim(o, SIM_NAMES, state, None, SIM_VS)
    for sim in (s, twin):
        for _ in range(2):  # (two core substeps with one dt: the second looks ahead, and its memo is pending while the points are sampled)
            sim.core_substep(3, 0.04, SIM_VS)
    now = download(s, SIM_NAMES)
    R = Rig(o, now["vel"], [now[k] for k in SIM_NAMES], SIM_VS)
    p = R.dev(xyz)
    got = s.sample(xyz=p, velocity=True)
    assert list(got) == SIM_NAMES + ["vel"]
    want = R.sample(R.phi + [R.vel], xyz, "sim")
    G = OracleGrid(o)
    for i, k in enumerate(got):
        assert_words(got[k].cpu().numpy(), want[i], f"Sim.sample: {k}")
    assert_words(want[0], G.sample_trilinear_f(now["density"], xyz), "Sim.sample: density against the oracle")
    some = s.sample(["flame", "density"], p)
    assert list(some) == ["flame", "density"]
    assert_words(some["flame"].cpu().numpy(), want[4], "Sim.sample: a named subset, flame")
    assert_words(some["density"].cpu().numpy(), want[0], "Sim.sample: a named subset, density")
    inv_dx = float(F(1.0) / F(SIM_VS))
    for order, steps, dt in ((2, 1, 0.04), (4, 3, -0.04), (1, 2, 0.04)):
        q = R.dev(xyz)
        st = s.trace(q, dt=dt, voxel_size=SIM_VS, order=order, steps=steps, status=True)
        wq, wst = R.trace(R.vel, xyz, dt, inv_dx, order, steps, "sim")
        assert_words(q.cpu().numpy(), wq, f"Sim.trace order {order}")
        assert np.array_equal(st.cpu().numpy(), wst) and wst.any() and not wst.all()
        path, status = pc.trace_mirror(G, now["vel"], xyz, dt, inv_dx, order, steps)
        assert_words(wq, path[-1], f"Sim.trace order {order} against the mirror")
        assert s.trace(R.dev(xyz), dt=dt, voxel_size=SIM_VS, order=order, steps=steps) is None
    # the sim is as its twin, which was never sampled: fields, masks, what it looked ahead, and the next substep
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
    # after a regrid the calls read the new grid
    keep = s.regrid(1)
    o2 = np.ascontiguousarray(s.grid.coords()[::512], dtype=np.int32)
    assert len(o2) > len(o)
    now2 = download(s, SIM_NAMES)
    xyz2 = pc.make_points(o2, 77, 1000)
    G2 = OracleGrid(o2)
    assert (pc.taps_inside(G2, xyz2) == 8).mean() > 0.3 and (pc.taps_inside(G, xyz2) != pc.taps_inside(G2, xyz2)).mean() > 0.1  # (points the old grid answers differently)
    got2 = s.sample(["temperature"], R.dev(xyz2), velocity=True)
    assert_words(got2["temperature"].cpu().numpy(), G2.sample_trilinear_f(now2["temperature"], xyz2), "after a regrid: temperature")
    with pc.fma_branch():
        assert_words(got2["vel"].cpu().numpy(), G2.sample_trilinear_v(now2["vel"], xyz2), "after a regrid: velocity")
    q = R.dev(xyz2)
    st = s.trace(q, dt=0.04, voxel_size=SIM_VS, order=4, steps=2, status=True)
    path, status = pc.trace_mirror(G2, now2["vel"], xyz2, 0.04, inv_dx, 4, 2)
    assert_words(q.cpu().numpy(), path[-1], "after a regrid: traced positions")
    assert np.array_equal(st.cpu().numpy(), status)
    del keep
    s.close(), twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------


def test_refusals_name_the_call_and_touch_nothing():
    from hnanosolver_amd import _lib

    lib = _lib.load_library()
    R = rig("ragged32")
    t, n = R.t, 65
    xyz_np = pc.case("ragged32")[3][:n]
    xyz = R.dev(xyz_np)
    out = [t.full((n,), float(SENTINEL), dtype=t.float32, device="cuda"), t.full((n, 3), float(SENTINEL), dtype=t.float32, device="cuda")]
    status = t.full((n,), STATUS_SENTINEL, dtype=t.uint8, device="cuda")
    state = random_state(3, len(R.o), SIM_NAMES + ["collision_sdf"])
    g, s = make_sim(R.o, SIM_NAMES + ["collision_sdf"], state, None, SIM_VS)
    P = lambda *a: (C.c_void_p * len(a))(*a)
    I = lambda *a: (C.c_int * len(a))(*a)
    S = lambda *a: (C.c_char_p * len(a))(*a)
    f0, v0, o0, o1, x, st, G = R.phi[0].data_ptr(), R.vel.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), xyz.data_ptr(), status.data_ptr(), R.grid.ptr
    nan, inf = float("nan"), float("inf")

    def ds(fields=P(f0, v0), ncomp=I(1, 3), k=2, p=x, count=n, outs=P(o0, o1)):
        return lambda: lib.hns_dev_sample_points(G, fields, ncomp, k, p, count, outs, None)

    def dt_(vel=v0, p=x, count=n, dt=0.04, inv=24.0, order=2, steps=1, status_=st):
        return lambda: lib.hns_dev_trace_points(G, vel, p, count, dt, inv, order, steps, status_, None)

    def ss(names=S(b"density"), k=1, vel=1, p=x, count=n, outs=P(o0, o1)):
        return lambda: lib.hns_sim_sample_points(s._ptr, names, k, vel, p, count, outs, None)

    def st_(p=x, count=n, dt=0.04, vs=SIM_VS, order=2, steps=1, status_=st):
        return lambda: lib.hns_sim_trace_points(s._ptr, p, count, dt, vs, order, steps, status_, None)

    rows = [
        ("hns_dev_sample_points", ds(p=None), "xyz"), ("hns_dev_sample_points", ds(fields=None), "list"), ("hns_dev_sample_points", ds(ncomp=None), "list"),
        ("hns_dev_sample_points", ds(outs=None), "list"), ("hns_dev_sample_points", ds(fields=P(f0, None)), "fields[1]"), ("hns_dev_sample_points", ds(outs=P(None, o1)), "out[0]"),
        ("hns_dev_sample_points", ds(ncomp=I(1, 2)), "ncomp[1]"), ("hns_dev_sample_points", ds(ncomp=I(0, 3)), "ncomp[0]"), ("hns_dev_sample_points", ds(k=0), "n_fields"),
        ("hns_dev_sample_points", ds(k=-1), "n_fields"), ("hns_dev_sample_points", ds(fields=P(f0, f0), ncomp=I(1, 1), outs=P(o0, o0)), "out[1] is out[0]"),
        ("hns_dev_sample_points", ds(outs=P(o0, x)), "out[1] is xyz"), ("hns_dev_sample_points", ds(outs=P(v0, o1)), "out[0] is fields[1]"),
        ("hns_dev_sample_points", ds(count=2 ** 31), "2^31"),
        ("hns_dev_trace_points", dt_(p=None), "xyz"), ("hns_dev_trace_points", dt_(vel=None), "vel3"), ("hns_dev_trace_points", dt_(order=3), "order"),
        ("hns_dev_trace_points", dt_(order=0), "order"), ("hns_dev_trace_points", dt_(steps=0), "steps"), ("hns_dev_trace_points", dt_(steps=-2), "steps"),
        ("hns_dev_trace_points", dt_(dt=nan), "dt"), ("hns_dev_trace_points", dt_(inv=0.0), "inv_dx"), ("hns_dev_trace_points", dt_(inv=-24.0), "inv_dx"),
        ("hns_dev_trace_points", dt_(inv=inf), "inv_dx"), ("hns_dev_trace_points", dt_(inv=nan), "inv_dx"), ("hns_dev_trace_points", dt_(count=2 ** 31), "2^31"),
        ("hns_dev_trace_points", dt_(status_=x), "status"),
        ("hns_sim_sample_points", ss(k=-2), "n_names"), ("hns_sim_sample_points", ss(names=S(b"smoke")), "'smoke'"), ("hns_sim_sample_points", ss(names=None), "names"),
        ("hns_sim_sample_points", ss(names=S(b"density", b"density"), k=2, outs=P(o0, o0, o1)), "twice"), ("hns_sim_sample_points", ss(k=0, vel=0), "no field"),
        ("hns_sim_sample_points", ss(p=None), "xyz"), ("hns_sim_sample_points", ss(outs=P(o0, x)), "out[1] is xyz"), ("hns_sim_sample_points", ss(outs=P(o0, o0)), "out[1] is out[0]"),
        ("hns_sim_sample_points", ss(outs=None), "list"), ("hns_sim_sample_points", ss(count=2 ** 31), "2^31"),
        ("hns_sim_trace_points", st_(p=None), "xyz"), ("hns_sim_trace_points", st_(vs=0.0), "voxel_size"), ("hns_sim_trace_points", st_(vs=-1.0), "voxel_size"),
        ("hns_sim_trace_points", st_(vs=inf), "voxel_size"), ("hns_sim_trace_points", st_(vs=nan), "voxel_size"), ("hns_sim_trace_points", st_(order=3), "order"),
        ("hns_sim_trace_points", st_(steps=0), "steps"), ("hns_sim_trace_points", st_(dt=nan), "dt"), ("hns_sim_trace_points", st_(count=2 ** 31), "2^31"),
        ("hns_sim_sample_points", lambda: lib.hns_sim_sample_points(None, S(b"density"), 1, 0, x, n, P(o0), None), "null sim"),
        ("hns_sim_trace_points", lambda: lib.hns_sim_trace_points(None, x, n, 0.04, SIM_VS, 2, 1, None, None), "null sim"),
        ("hns_dev_sample_points", lambda: lib.hns_dev_sample_points(None, P(f0), I(1), 1, x, n, P(o0), None), "null grid"),
        ("hns_dev_trace_points", lambda: lib.hns_dev_trace_points(None, v0, x, n, 0.04, 24.0, 2, 1, None, None), "null grid"),
    ]
    wrong = []
    for i, (call, fn, word) in enumerate(rows):
        lib.hns_set_option(b"rbgs", None)  # (a call that succeeds: whatever it leaves in hns_last_error(), the text read below is this row's)
        code, text = fn(), lib.hns_last_error().decode()
        if code != _lib.HNS_ERR_INVALID_ARGUMENT or not text.startswith(call + ":") or word not in text:
            wrong.append(f"row {i} {call} (expects {word!r}): got {code} {text!r}")
    t.cuda.synchronize()
    assert not wrong, "\n".join(wrong)
    assert all((words(o.cpu().numpy()) == 0xDEADBEEF).all() for o in out) and (status.cpu().numpy() == STATUS_SENTINEL).all(), "a refused call wrote an output"
    assert_words(xyz.cpu().numpy(), xyz_np, "a refused call moved the positions")
    # what is allowed: collision_sdf as any float field, one field listed twice as an input of the device call, n = 0 with nothing launched
    assert lib.hns_sim_sample_points(s._ptr, S(b"collision_sdf"), 1, 0, x, n, P(o0), None) == 0
    assert_words(out[0].cpu().numpy(), OracleGrid(R.o).sample_trilinear_f(state["collision_sdf"], xyz_np), "collision_sdf sampled as a float field")
    out[0].fill_(float(SENTINEL))
    assert ds(fields=P(f0, f0), ncomp=I(1, 1), count=0)() == 0 and dt_(count=0)() == 0 and ss(count=0)() == 0 and st_(count=0)() == 0
    t.cuda.synchronize()
    assert all((words(o.cpu().numpy()) == 0xDEADBEEF).all() for o in out) and (status.cpu().numpy() == STATUS_SENTINEL).all(), "a call with n = 0 wrote"
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. pool contents
# ---------------------------------------------------------------------------------------------------------------


def test_results_do_not_depend_on_what_pooled_memory_held():
    from pool_cases import arena_fill

    o, vel, phi, xyz = pc.case("sparse_far")
    state = {"vel": np.array(vel), "density": np.array(phi[0]), "flame": np.array(phi[1])}
    u = pc.scaled_velocity(vel, 4.0, F(pc.DT) * F(pc.INV_DX))

    def scenario():
        """a grid and a sim made now -- their tables and buffers come out of the pool -- sampled and traced"""
        R = Rig(o, u, phi[:2])
        g, s = make_sim(o, ["density", "flame"], state, None, SIM_VS)
        got = R.sample([R.phi[0], R.vel, R.phi[1]], xyz, "pool")
        pos, st = R.trace(R.vel, xyz, pc.DT, pc.INV_DX, 4, 3, "pool")
        p = R.dev(xyz)
        on_sim = s.sample(xyz=p, velocity=True)
        st2 = s.trace(p, dt=pc.DT, voxel_size=SIM_VS, order=2, steps=2, status=True)
        res = [*got, pos, st, *[v.cpu().numpy() for v in on_sim.values()], p.cpu().numpy(), st2.cpu().numpy()]
        s.close()
        return [np.ascontiguousarray(a).tobytes() for a in res]

    base = scenario()
    for fill in (255, 127):
        with arena_fill(fill):
            got = scenario()
        assert len(got) == len(base) and all(a == b for a, b in zip(got, base)), f"arena_fill {fill}: outputs {[i for i, (a, b) in enumerate(zip(got, base)) if a != b]} differ"
