"""advect_scalar over many fields with one back-trace: hns_dev_advect_scalar_multi (k_advect_scalar_multi_n), hns_sim_advect and the AdvectIndexGrid operator on top.

Every output is held to one single-field launch per field (hns_dev_advect_scalar, k_advect_scalar_n) as raw 32-bit words, to the reference's own advect_scalar body,
to the device-semantics oracle on special values and to the oracle's restated AdvectIndexGrid driver. Nothing here is a tolerance: every comparison is equality
of bit patterns (a NaN against a NaN where the special-value tests say so)."""
import functools

import numpy as np
import pytest

import special_cases as sc
from frame_cases import download, make_sim
from hnanosolver_amd import fields

pytestmark = pytest.mark.gpu

DT = float(np.float32(1.0 / 24.0))
SENTINEL = np.frombuffer(np.uint32(0xDEADBEEF).tobytes(), np.float32)[0]  # what an output buffer holds before a call


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def assert_words(got, want, what):
    """equal as 32-bit words: zero signs, subnormals, inf, and the sign and payload of every NaN"""
    g, w = words(got), words(want)
    d = np.flatnonzero(g != w)
    assert len(d) == 0, f"{what}: {len(d)} of {g.size} words differ; first at {d[:6].tolist()}: {[hex(x) for x in g[d[:6]]]} vs {[hex(x) for x in w[d[:6]]]}"


@pytest.fixture(autouse=True)
def _default_options():
    import hnanosolver_amd as H

    yield
    for k in ("lookahead", "advect"):
        H.set_option(k, None)


class Kernels:
    """one launch per field and the shared back-trace, on device copies of the same host arrays; outputs start as SENTINEL"""

    def __init__(self, origins, vs):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.grid = api.create_grid_from_leaves(np.ascontiguousarray(origins, dtype=np.int32), vs)

    def dev(self, a):
        return None if a is None else self.t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def blank(self, like):
        return self.t.full_like(like, float(SENTINEL))

    def single(self, vel, phis, dt, inv_dx, sdf=None, coll=False):
        u, s, out = self.dev(vel), self.dev(sdf), []
        for p in phis:
            src = self.dev(p)
            out.append(self.D.advect_scalar(self.grid, u, src, self.blank(src), dt, inv_dx, s, coll).cpu().numpy())
        return out

    def multi(self, vel, phis, dt, inv_dx, sdf=None, coll=False):
        u = self.dev(vel)
        src = [self.dev(p) for p in phis]
        dst = [self.blank(p) for p in src]
        self.D.advect_scalar_multi(self.grid, u, src, dst, dt, inv_dx, self.dev(sdf), coll)
        return [d.cpu().numpy() for d in dst]


# ---------------------------------------------------------------------------------------------------------------
# 1. against the single-field HIP kernel
# ---------------------------------------------------------------------------------------------------------------

GRIDS = {
    "ragged32": lambda: sc.ragged32(),
    "ragged32_shifted": lambda: sc.ragged32(shift=(3 * 8, -5 * 8, 6 * 8)),  # by (3, -5, 6) leaves: origins stay 8-aligned, no leaf near (0, 0, 0)
    "sparse_far": sc.sparse_far,
    "one_leaf": sc.LEAF_SETS["one_leaf"],
    "dense32": lambda: fields.dense_leaves(32),
}
VS = 1.0 / 48.0
INV = float(np.float32(1.0) / np.float32(VS))
S_LIST = (1, 2, 8, 9, 11)  # both sides of the split at eight fields per launch


@functools.lru_cache(maxsize=None)
def random_case(grid, speed):
    """velocity with back-traces of about `speed` voxels, eleven random fields, a collision SDF and the single-field kernel's result per field, computed once"""
    o = np.ascontiguousarray(GRIDS[grid](), dtype=np.int32)
    rng = np.random.default_rng([17, list(GRIDS).index(grid), int(speed)])
    N = len(o) * 512
    vel = (rng.standard_normal((N, 3)) * (speed * VS / DT / 2.0)).astype(np.float32)
    phi = [rng.standard_normal(N).astype(np.float32) for _ in range(11)]
    sdf = (rng.standard_normal(N) * 0.5).astype(np.float32)
    sdf[rng.random(N) < 0.2] = np.float32(0.05)
    K = Kernels(o, VS)
    return K, vel, phi, sdf, K.single(vel, phi, DT, INV)


@pytest.mark.parametrize("speed", [4.0, 9.0, 30.0])  # near path, two-hop, origin hash
@pytest.mark.parametrize("grid", list(GRIDS))
def test_equals_one_launch_per_field(grid, speed):
    K, vel, phi, _, want = random_case(grid, speed)
    for S in S_LIST:
        got = K.multi(vel, phi[:S], DT, INV)
        assert len(got) == S
        for i in range(S):
            assert_words(got[i], want[i], f"{grid} speed {speed} S={S} field {i}")
    assert K.multi(vel, [], DT, INV) == []  # n = 0 is a call like any other


@pytest.mark.parametrize("grid", ["ragged32", "sparse_far"])
def test_the_same_input_listed_twice(grid):
    K, vel, phi, _, want = random_case(grid, 9.0)
    order = [0, 1, 0, 2, 2, 3, 4, 5, 0, 1]  # repeats inside one launch and across the split
    got = K.multi(vel, [phi[i] for i in order], DT, INV)
    for k, i in enumerate(order):
        assert_words(got[k], want[i], f"{grid}: output {k} (input {i})")


@pytest.mark.parametrize("grid", ["ragged32", "sparse_far"])
def test_option_advect_generic_gives_the_same_words(grid):
    import hnanosolver_amd as H

    K, vel, phi, _, want = random_case(grid, 9.0)
    H.set_option("advect", "generic")
    try:
        got = K.multi(vel, phi[:9], DT, INV)
    finally:
        H.set_option("advect", None)
    for i in range(9):
        assert_words(got[i], want[i], f"{grid} advect = generic field {i}")


@pytest.mark.parametrize("grid", ["ragged32", "sparse_far"])
def test_with_a_collision_field_it_is_one_launch_per_field(grid):
    K, vel, phi, sdf, plain = random_case(grid, 4.0)
    want = K.single(vel, phi[:9], DT, INV, sdf, True)
    assert any((words(a) != words(b)).any() for a, b in zip(want, plain))  # (the SDF does change the result)
    got = K.multi(vel, phi[:9], DT, INV, sdf, True)
    for i in range(9):
        assert_words(got[i], want[i], f"{grid} collision field {i}")


# ---------------------------------------------------------------------------------------------------------------
# 2. against the reference's own kernel body
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed,speed", [(31, 4.0), (32, 9.0), (33, 30.0)])
def test_equals_the_reference_kernel(seed, speed):
    from oracle_lib import RefKernelGrid, reference_kernels, reference_samplers
    from test_ref_kernels import _random_case
    from test_ref_kernels_gpu import same

    if reference_kernels() is None or reference_samplers() is None:
        pytest.skip("oracle/_ref/libhns_refk.so did not travel")
    rng, o = _random_case(seed)
    R, K = RefKernelGrid(o), Kernels(o, VS)
    N = R.N
    vel = (rng.standard_normal((N, 3)) * (speed * VS / DT / 2.0)).astype(np.float32)
    phi = [rng.standard_normal(N).astype(np.float32) for _ in range(11)]
    got = K.multi(vel, phi, DT, INV)
    for i in range(11):
        same(got[i], R.advect_scalar(vel, phi[i], DT, INV, None, False), f"seed {seed} speed {speed} field {i}")


# ---------------------------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("where", sc.WHERE)
@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("leaves", ["ragged32", "sparse_far"])
def test_special_values(leaves, cls, where):
    """signed zeros, subnormals, NaN, inf, overflow and threshold positions, S = 3: against the device-semantics oracle's advect_scalar (a NaN equal to any NaN) and
    against the single-field HIP kernel as raw words, where two NaN at the same position may differ in the sign bit alone (special_cases.nan_sign_differences)"""
    from oracle_lib import OracleGrid, oracle_device

    o = sc.LEAF_SETS[leaves]()
    w = sc.Workload(o, cls, where)
    K, D = Kernels(o, sc.VS), OracleGrid(o, lib=oracle_device())
    got = K.multi(w.vel, w.phi[:3], sc.DT, sc.INV)
    one = K.single(w.vel, w.phi[:3], sc.DT, sc.INV)
    for i in range(3):
        want = D.advect_scalar(w.vel, w.phi[i], sc.DT, sc.INV, None, False)
        assert sc.same_bits(got[i], want), f"field {i} vs the oracle: {sc.describe(got[i], want)}"
        ok, count = sc.nan_sign_differences(got[i], one[i])
        print(f"{leaves} {cls} {where} field {i}: {count} words differ from the single-field kernel (NaN signs only: {ok})")
        assert ok, f"field {i} vs the single-field kernel: {sc.describe(got[i], one[i])}"


# ---------------------------------------------------------------------------------------------------------------
# 4. launch range
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("S", [3, 9])
def test_launch_range(S):
    first, count = 5, 11
    o = sc.ragged32()
    rng = np.random.default_rng(23)
    N = len(o) * 512
    vel = (rng.standard_normal((N, 3)) * (9.0 * VS / DT / 2.0)).astype(np.float32)
    phi = [rng.standard_normal(N).astype(np.float32) for _ in range(S)]
    K = Kernels(o, VS)
    K.grid.set_active_range(first, count)
    got, want = K.multi(vel, phi, DT, INV), K.single(vel, phi, DT, INV)
    inside = slice(first * 512, (first + count) * 512)
    outside = np.ones(N, dtype=bool)
    outside[inside] = False
    for i in range(S):
        assert_words(got[i][inside], want[i][inside], f"S={S} field {i}: leaves of the range")
        assert (words(got[i])[outside] == 0xDEADBEEF).all(), f"S={S} field {i}: a word outside the range was written"
        assert (words(want[i])[outside] == 0xDEADBEEF).all()
    K.grid.set_active_range(0, len(o))
    whole = K.multi(vel, phi, DT, INV)
    for i in range(S):
        assert_words(whole[i][inside], got[i][inside], f"S={S} field {i}: the range against the whole grid")


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------


def test_refusals():
    from hnanosolver_amd._lib import lib

    o = sc.ragged32()
    K = Kernels(o, VS)
    N = len(o) * 512
    u = K.dev(np.zeros((N, 3)))
    p = [K.dev(np.full(N, float(i))) for i in range(10)]
    q = [K.blank(x) for x in p]
    u3 = K.blank(u)  # an "output" that is the velocity: same pointer, checked before anything is launched

    def refused(srcs, dsts, vel, text):
        with pytest.raises(ValueError, match=text):
            K.D.advect_scalar_multi(K.grid, vel, srcs, dsts, DT, INV)
        assert text.replace("\\", "") in lib.hns_last_error().decode()
        K.t.cuda.synchronize()
        for x in q + [u3]:
            assert (words(x.cpu().numpy()) == 0xDEADBEEF).all(), f"{text}: something was written"
        for i, x in enumerate(p):
            assert (x == float(i)).all()

    refused(p[:4], [q[0], q[1], p[3], q[3]], u, "output of field 2 aliases the input of field 3")
    refused(p[:4], [q[0], p[1], q[2], q[3]], u, "output of field 1 aliases the input of field 1")
    refused(p[:10], q[:9] + [p[0]], u, "output of field 9 aliases the input of field 0")  # across the split at eight
    refused(p[:3], [q[0], q[1], u3], u3, "output of field 2 aliases the velocity")
    refused(p[:4], [q[0], q[1], q[2], q[1]], u, "output of field 3 is the output of field 1")
    refused(p[:10], q[:9] + [q[2]], u, "output of field 9 is the output of field 2")
    refused([p[0], p[1], None, p[3]], q[:4], u, "null device pointer for field 2")
    refused(p[:10], q[:9] + [None], u, "null device pointer for field 9")
    with pytest.raises(ValueError, match="null device pointer"):
        K.D.advect_scalar_multi(K.grid, None, p[:1], q[:1], DT, INV)


# ---------------------------------------------------------------------------------------------------------------
# 6. Sim.advect
# ---------------------------------------------------------------------------------------------------------------

SIM_NAMES = ["density", "temperature", "fuel"]


def sim_state(o, seed=29):
    rng = np.random.default_rng(seed)
    N = len(o) * 512
    st = {"vel": (rng.standard_normal((N, 3)) * (4.0 / sc.SDT / 2.0)).astype(np.float32)}
    for n in SIM_NAMES:
        st[n] = rng.standard_normal(N).astype(np.float32)
    return st


def operators(o, st, names, velocity):
    """api.AdvectIndexGrid over `names`, then api.AdvectIndexGridVelocity: -> {name: array}"""
    from hnanosolver_amd import api

    d = api.GridIndexedData()
    c = fields.leaves_to_coords(o)
    d.allocateCoords(len(c))
    d.pCoords()[:] = c
    for n in names:
        d.addValueBlock(n, d.FLOAT)
        d.pValues(n)[:] = st[n]
    d.addValueBlock("vel", d.VEC3F)
    d.pValues("vel")[:] = st["vel"]
    if names:
        api.AdvectIndexGrid(d, sc.DT, sc.VS)
    if velocity:
        api.AdvectIndexGridVelocity(d, sc.DT, sc.VS)
    return {n: d.pValues(n).copy() for n in list(names) + ["vel"]}


@pytest.mark.parametrize("names,velocity", [(["fuel", "density"], True), (None, False), (None, True), ([], True)])
def test_sim_advect_equals_the_two_operators(names, velocity):
    o = sc.ragged32()
    st = sim_state(o)
    g, s = make_sim(o, SIM_NAMES, st, None, sc.VS)
    s.advect(names, velocity, dt=sc.DT, voxel_size=sc.VS)
    got = download(s, SIM_NAMES)
    s.close()
    advected = SIM_NAMES if names is None else names
    want = operators(o, st, advected, velocity)
    for n in SIM_NAMES:
        if n in advected:
            assert (words(want[n]) != words(st[n])).any()
        assert_words(got[n], want[n] if n in advected else st[n], f"names {names} velocity {velocity}: {n}")
    assert_words(got["vel"], want["vel"], f"names {names} velocity {velocity}: vel")
    assert (words(want["vel"]) != words(st["vel"])).any() == velocity


def test_sim_advect_refusals_change_nothing():
    from hnanosolver_amd._lib import lib

    o = sc.ragged32()
    st = sim_state(o)
    g, s = make_sim(o, SIM_NAMES, st, None, sc.VS)
    for names, text in ((["density", "smoke"], "no float field named 'smoke'"), (["fuel", "density", "fuel"], "field 'fuel' is listed twice")):
        with pytest.raises(ValueError, match=text):
            s.advect(names, True, dt=sc.DT, voxel_size=sc.VS)
        assert lib.hns_last_error().decode().startswith("hns_sim_advect:")
        got = download(s, SIM_NAMES)
        for k in got:
            assert_words(got[k], st[k], f"refused {names}: {k}")
    with pytest.raises(ValueError, match="voxelSize must be positive"):
        s.advect(None, True, dt=sc.DT, voxel_size=0.0)
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the look-ahead memo
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("velocity", [True, False])
def test_lookahead_memo_across_sim_advect(velocity):
    """lookahead = 1: the second core substep leaves advect_vector(vel) in adv. Sim.advect(velocity=True) overwrites adv and vel, so the memo must be dropped -- the
    substep behind it gives the bits of lookahead = 0. With velocity=False neither buffer is written and the result is the same either way."""
    from test_lookahead_gpu import ITERS
    from test_lookahead_gpu import VS as LVS
    from test_lookahead_gpu import assert_same_runs, run

    def script(s, snap):
        s.core_substep(ITERS, DT, LVS), s.core_substep(ITERS, DT, LVS)
        s.advect(None, velocity, dt=DT, voxel_size=LVS)
        snap()
        s.core_substep(ITERS, DT, LVS)

    want, c0 = run("0", ["density"], script)
    got, c1 = run("1", ["density"], script)
    assert c0 == (0, 0) and c1[0] >= 2  # (the case did look ahead before the call)
    assert_same_runs(got, want, f"lookahead = 1 across advect(velocity={velocity})")


# ---------------------------------------------------------------------------------------------------------------
# 8. the operator
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_fields", [1, 3, 9])
def test_operator_equals_the_oracle_driver(n_fields):
    """api.AdvectIndexGrid against the oracle's restated driver (one advect_scalar per float block, Advection.cu:88-91), bit for bit"""
    from hnanosolver_amd import api
    from oracle_lib import OracleGrid
    from test_ref_kernels import _random_case

    rng, o = _random_case(41, span=2, keep=0.6)
    R = 32
    vs = 1.0 / R
    N = len(o) * 512
    vel = (rng.standard_normal((N, 3)) * (4.0 * vs / DT / 2.0)).astype(np.float32)
    phi = [rng.standard_normal(N).astype(np.float32) for _ in range(n_fields)]
    want = [p.copy() for p in phi]
    assert OracleGrid(o).advect_index_grid(vel.copy(), want, DT, vs) == 0
    d = api.GridIndexedData()
    c = fields.leaves_to_coords(o)
    d.allocateCoords(len(c))
    d.pCoords()[:] = c
    for i, p in enumerate(phi):
        d.addValueBlock(f"f{i}", d.FLOAT)
        d.pValues(f"f{i}")[:] = p
    d.addValueBlock("vel", d.VEC3F)
    d.pValues("vel")[:] = vel
    api.AdvectIndexGrid(d, DT, vs)
    for i in range(n_fields):
        assert (words(want[i]) != words(phi[i])).any()
        assert_words(d.pValues(f"f{i}"), want[i], f"{n_fields} fields: f{i}")
    assert_words(d.pValues("vel"), vel, "the velocity block is left as it was")
