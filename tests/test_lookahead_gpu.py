"""Look-ahead: a substep's advect_scalars launch also computes the next substep's advect_vector (option "lookahead").

Kernel level: hns_dev_advect_scalars_ahead against hns_dev_advect_scalars followed by hns_dev_advect_vector, as 32-bit words (a NaN
against the same NaN), on every field and on the advected velocity; both against the oracle where the parity and special-value
tests compare with it. Substep level: lookahead = 1 and auto against lookahead = 0 after every substep. Invalidation: one case per
writer of the velocity, each against lookahead = 0. Nothing here is a tolerance: every comparison is equality of bit patterns."""
import functools

import numpy as np
import pytest

import special_cases as sc
from frame_cases import COMBUST, download, emitter, make_sim
from hnanosolver_amd import fields

pytestmark = pytest.mark.gpu

DT = float(np.float32(1.0 / 24.0))


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def assert_words(got, want, what):
    """equal as 32-bit words: zero signs, subnormals, inf, and the sign and payload of every NaN"""
    g, w = words(got), words(want)
    d = np.flatnonzero(g != w)
    print(f"{what}: {len(d)} of {g.size} words differ")
    assert len(d) == 0, f"{what}: {len(d)} of {g.size} words differ; first at {d[:6].tolist()}: {[hex(x) for x in g[d[:6]]]} vs {[hex(x) for x in w[d[:6]]]}"


@pytest.fixture(autouse=True)
def _default_options():
    import hnanosolver_amd as H

    yield
    for k in ("lookahead", "fuse", "advect"):
        H.set_option(k, None)


class Kernels:
    """the two launches and the one, on device copies of the same host arrays"""

    def __init__(self, origins, vs):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.grid = api.create_grid_from_leaves(np.ascontiguousarray(origins, dtype=np.int32), vs)

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def separate(self, vel, phis, dt, inv_dx):
        u, src = self.dev(vel), [self.dev(p) for p in phis]
        dst, adv = [self.t.full_like(p, 7.0) for p in src], self.t.full_like(u, 7.0)
        self.D.advect_scalars(self.grid, u, src, dst, dt, inv_dx)
        self.D.advect_vector(self.grid, u, adv, dt, inv_dx)
        return [d.cpu().numpy() for d in dst], adv.cpu().numpy()

    def fused(self, vel, phis, dt, inv_dx):
        u, src = self.dev(vel), [self.dev(p) for p in phis]
        dst, adv = [self.t.full_like(p, -7.0) for p in src], self.t.full_like(u, -7.0)
        self.D.advect_scalars_ahead(self.grid, u, src, dst, adv, dt, inv_dx)
        return [d.cpu().numpy() for d in dst], adv.cpu().numpy()

    def check(self, vel, phis, dt, inv_dx, what):
        got, got_adv = self.fused(vel, phis, dt, inv_dx)
        want, want_adv = self.separate(vel, phis, dt, inv_dx)
        assert_words(got_adv, want_adv, f"{what}: adv_out")
        for i, (a, b) in enumerate(zip(got, want)):
            assert_words(a, b, f"{what}: field {i}")
        return got, got_adv


GRIDS = {
    "dense64": lambda: (fields.dense_leaves(64), 64),
    "dense128": lambda: (fields.dense_leaves(128), 128),
    "plume": lambda: fields.config_leaves("plume"),  # 3.9k leaves: absent neighbours and domain faces
}


@functools.lru_cache(maxsize=2)
def big_case(name, amplitude):
    o, R = GRIDS[name]()
    f = fields.synthetic_fields(o, R, amplitude_voxels=amplitude)
    rng = np.random.default_rng(11)
    N = len(o) * 512
    vel = (f["vel"] + 0.05 * np.abs(f["vel"]).max() * rng.standard_normal((N, 3))).astype(np.float32)
    vel[0] = np.float32(amplitude / R) * np.array([0.75, -0.5, 0.375], dtype=np.float32)  # element 0: what advect_scalars samples outside the domain, advect_vector samples 0
    phis = [f[n].copy() for n in COMBUST] + [rng.standard_normal(N).astype(np.float32) for _ in range(3)]
    phis[0][0] = 100.0
    return Kernels(o, 1.0 / R), R, vel, phis


@pytest.mark.parametrize("S", [1, 5, 8])
@pytest.mark.parametrize("amplitude", [96.0, 400.0])  # 400: the taps reach beyond the 27-leaf neighbourhood
@pytest.mark.parametrize("grid", list(GRIDS))
def test_one_launch_equals_the_two(grid, amplitude, S):
    K, R, vel, phis = big_case(grid, amplitude)
    K.check(vel, phis[:S], DT, float(np.float32(R)), f"{grid} A={amplitude} S={S}")


@pytest.mark.parametrize("name", ["dense16", "dense32", "sparse", "plume_small"])
def test_one_launch_equals_the_oracle(name):
    """the cases of tests/test_parity_gpu.py, bit for bit against the CPU oracle's advect_scalars and advect_vector"""
    from oracle_lib import OracleGrid
    from test_parity_gpu import CASES

    o, R = CASES[name]()
    f = fields.synthetic_fields(o, R)
    rng = np.random.default_rng(0)
    for k in f:
        f[k] = (f[k] + 0.05 * rng.standard_normal(f[k].shape) * max(1e-3, np.abs(f[k]).max())).astype(np.float32)
    phis = [f[n].copy() for n in COMBUST]
    phis[0][0] = 100.0
    K, G = Kernels(o, 1.0 / R), OracleGrid(o)
    inv_dx = float(np.float32(1.0) / np.float32(1.0 / R))
    for S in (1, 5):
        got, got_adv = K.check(f["vel"], phis[:S], DT, inv_dx, f"{name} S={S}")
        want = G.advect_scalars(f["vel"], phis[:S], DT, inv_dx)
        for i in range(S):
            assert np.array_equal(got[i], want[i]), f"{name} S={S} field {i}: not bit-identical to the oracle"
        assert np.array_equal(got_adv, G.advect_vector(f["vel"], DT, inv_dx)), f"{name} S={S} adv_out: not bit-identical to the oracle"


@pytest.mark.parametrize("where", sc.WHERE)
@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("leaves", list(sc.LEAF_SETS))
def test_special_values(leaves, cls, where):
    """signed zeros, subnormals, NaN, inf, overflow and threshold positions: the one launch against the two as words, and against
    the device-semantics oracle as the special-value tests compare (a NaN equal to any NaN)"""
    from oracle_lib import OracleGrid, oracle_device

    o = sc.LEAF_SETS[leaves]()
    w = sc.Workload(o, cls, where)
    K, D = Kernels(o, sc.VS), OracleGrid(o, lib=oracle_device())
    want_adv = D.advect_vector(w.vel, sc.DT, sc.INV, None, False)
    for S in (1, 5, 8):
        got, got_adv = K.check(w.vel, w.phi[:S], sc.DT, sc.INV, f"{leaves} {cls} {where} S={S}")
        want = D.advect_scalars(w.vel, w.phi[:S], sc.DT, sc.INV, None, False)
        for i in range(S):
            assert sc.same_bits(got[i], want[i]), f"S={S} field {i} vs the oracle: {sc.describe(got[i], want[i])}"
        assert sc.same_bits(got_adv, want_adv), f"S={S} adv_out vs the oracle: {sc.describe(got_adv, want_adv)}"


@pytest.mark.parametrize("leaves", ["ragged32", "ragged32_off_origin", "sparse_far"])
@pytest.mark.parametrize("cls", ["zeros", "nonfinite"])
def test_special_values_on_long_back_traces(leaves, cls):
    o = sc.LEAF_SETS[leaves]()
    w = sc.Workload(o, cls, "both", seed=1, speed=30.0)
    Kernels(o, sc.VS).check(w.vel, w.phi[:5], sc.DT, sc.INV, f"{leaves} {cls} speed 30")


def test_refusals():
    import hnanosolver_amd as H

    o = fields.dense_leaves(16)
    K = Kernels(o, 1.0 / 16)
    u = K.dev(np.zeros((len(o) * 512, 3)))
    p = [K.dev(np.zeros(len(o) * 512)) for _ in range(9)]
    q = [K.t.empty_like(x) for x in p]
    # HNS_ERR_INVALID_ARGUMENT reaches Python as ValueError (api._raise)
    with pytest.raises(ValueError, match="between 0 and 8 fields"):
        K.D.advect_scalars_ahead(K.grid, u, p, q, K.t.empty_like(u), DT, 16.0)
    with pytest.raises(ValueError, match="must not alias"):
        K.D.advect_scalars_ahead(K.grid, u, p[:1], q[:1], u, DT, 16.0)
    H.set_option("advect", "generic")
    with pytest.raises(ValueError, match="32-bit offsets"):
        K.D.advect_scalars_ahead(K.grid, u, p[:1], q[:1], K.t.empty_like(u), DT, 16.0)  # the 64-bit kernels have no look-ahead form


# ---------------------------------------------------------------------------------------------------------------
# substeps
# ---------------------------------------------------------------------------------------------------------------

R = 32
VS = 1.0 / R
ITERS = 4


def start_state(names, seed=2):
    o = fields.dense_leaves(R)
    f = fields.synthetic_fields(o, R)
    rng = np.random.default_rng(seed)
    st = {"vel": (f["vel"] + 0.02 * rng.standard_normal(f["vel"].shape)).astype(np.float32)}
    for n in names:
        st[n] = fields.sphere_sdf(o, R, center=(0.4, 0.5, 0.5), radius=0.2) if n == "collision_sdf" else (f[n] + 0.01 * rng.standard_normal(len(o) * 512)).astype(np.float32)
    return o, st


def run(mode, names, script, fuse=None):
    """`script(sim, snap)` under lookahead = mode on a fresh sim; snap() downloads the velocity and every field: -> (snapshots, counts)"""
    import hnanosolver_amd as H

    H.set_option("lookahead", mode)
    if fuse is not None:
        H.set_option("fuse", fuse)
    o, st = start_state(names)
    g, s = make_sim(o, names, st, None, VS)
    snaps = []

    def snap():
        snaps.append(download(s, names))

    script(s, snap)
    snap()
    counts = s.lookahead_counts()
    s.close()
    return snaps, counts


def assert_same_runs(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k].shape == y[k].shape, f"{what}: snapshot {i} field {k}: shapes differ"
            assert_words(x[k], y[k], f"{what}: snapshot {i} field {k}")


def core_steps(n, with_download):
    def script(s, snap):
        for _ in range(n):
            s.core_substep(ITERS, DT, VS)
            if with_download:
                snap()

    return script


def full_steps(n, with_download, params):
    def script(s, snap):
        for _ in range(n):
            s.substep(ITERS, DT, VS, params, False)
            if with_download:
                snap()

    return script


@pytest.mark.parametrize("with_download", [True, False])
def test_core_substeps(with_download):
    want, c0 = run("0", ["density"], core_steps(6, with_download))
    assert c0 == (0, 0)
    got1, c1 = run("1", ["density"], core_steps(6, with_download))
    assert c1 == (6, 5)  # every substep looks ahead, every substep but the first finds its advect_vector done
    assert_same_runs(got1, want, f"core, lookahead = 1, download {with_download}")
    gota, ca = run("auto", ["density"], core_steps(6, with_download))
    assert ca == (5, 4)  # auto: from the second substep with the same dt and voxel size
    assert_same_runs(gota, want, f"core, lookahead = auto, download {with_download}")


@pytest.mark.parametrize("vorticity", [False, True])
@pytest.mark.parametrize("with_download", [True, False])
def test_full_substeps_unfused(with_download, vorticity):
    from hnanosolver_amd import api

    p = api.CombustionParams(factorScale=1.0, vorticityScale=0.4) if vorticity else api.CombustionParams()
    want, c0 = run("0", COMBUST, full_steps(6, with_download, p), fuse="0")
    assert c0 == (0, 0)
    for mode, counts in (("1", (6, 5)), ("auto", (5, 4))):
        got, c = run(mode, COMBUST, full_steps(6, with_download, p), fuse="0")
        assert c == counts
        assert_same_runs(got, want, f"S = 5, fuse = 0, lookahead = {mode}, download {with_download}, vorticity {vorticity}")


def test_fused_substep_is_unaffected():
    from hnanosolver_amd import api

    p = api.CombustionParams()
    want, c0 = run("0", COMBUST, full_steps(6, True, p), fuse="1")
    got, c1 = run("1", COMBUST, full_steps(6, True, p), fuse="1")
    assert c0 == (0, 0) and c1 == (0, 0)  # the q4 form of part C keeps its two launches
    assert_same_runs(got, want, "fuse = 1")


# ---------------------------------------------------------------------------------------------------------------
# invalidation: one case per writer of the velocity, each against lookahead = 0
# ---------------------------------------------------------------------------------------------------------------


def operator_data(s, n_extra=()):
    from hnanosolver_amd import api

    c = s.grid.coords()
    d = api.GridIndexedData()
    d.allocateCoords(len(c))
    d.pCoords()[:] = c
    for n in n_extra:
        d.addValueBlock(n, d.FLOAT)
        d.pValues(n)[:] = 0.0
    d.addValueBlock("vel", d.VEC3F)
    d.pValues("vel")[:] = np.random.default_rng(9).standard_normal((len(c), 3)).astype(np.float32)
    return d


def sc_upload(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    n = s.grid.voxel_count()
    s.upload({"vel": (0.3 * np.random.default_rng(4).standard_normal((n, 3))).astype(np.float32)})
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS)


def sc_upload_field_only(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    s.upload({"density": np.random.default_rng(4).random(s.grid.voxel_count()).astype(np.float32)})
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS)


def sc_dt(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    s.core_substep(ITERS, DT / 2, VS), snap(), s.core_substep(ITERS, DT / 2, VS), snap(), s.core_substep(ITERS, DT, VS)


def sc_voxel_size(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    s.core_substep(ITERS, DT, VS * 1.5), snap(), s.core_substep(ITERS, DT, VS * 1.5), snap(), s.core_substep(ITERS, DT, VS)


def sc_regrid(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    s.regrid(2)
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS)


def sc_regrid_sourced(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    src = emitter(R, 0)
    s.regrid(1, sources={"vel": src["vel"], "density": src["density"]})
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS)


def sc_deactivate(s, snap):
    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    s.deactivate({"density": 1e-3}, velocity=0.5)
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS)
    s.regrid(1)
    s.core_substep(ITERS, DT, VS)


def sc_divergence_operator(s, snap):
    from hnanosolver_amd import api

    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    api.Divergence(operator_data(s, ("divergence",)), VS, handle=s.grid)
    s.core_substep(ITERS, DT, VS), snap()
    api.ProjectNonDivergent(operator_data(s), 3, VS, handle=s.grid)
    api.AdvectIndexGridVelocity(operator_data(s), DT, VS, handle=s.grid)
    s.core_substep(ITERS, DT, VS)


def sc_velocity_ptr(s, snap):
    import torch

    from hnanosolver_amd._lib import lib

    s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    n = s.grid.voxel_count()
    new = torch.from_numpy((0.3 * np.random.default_rng(6).standard_normal((n, 3))).astype(np.float32)).cuda()
    ids = torch.arange(n // 512, dtype=torch.int32, device="cuda")
    ptr = s.velocity_ptr()
    assert ptr
    assert lib.hns_dev_unpack_leaves(new.data_ptr(), ids.data_ptr(), n // 512, ptr, 3, 0) == 0  # the caller's own kernel writing through the pointer
    torch.cuda.synchronize()
    before = s.lookahead_counts()
    s.core_substep(ITERS, DT, VS), snap(), s.core_substep(ITERS, DT, VS), s.core_substep(ITERS, DT, VS)
    assert s.lookahead_counts() == before  # off for good


INVALIDATORS = {"upload": sc_upload, "upload_field_only": sc_upload_field_only, "dt": sc_dt, "voxel_size": sc_voxel_size, "regrid": sc_regrid, "regrid_sourced": sc_regrid_sourced,
                "deactivate": sc_deactivate, "operators": sc_divergence_operator, "velocity_ptr": sc_velocity_ptr}


@pytest.mark.parametrize("mode", ["1", "auto"])
@pytest.mark.parametrize("writer", list(INVALIDATORS))
def test_writers_of_the_velocity_drop_what_was_looked_ahead(writer, mode):
    want, _ = run("0", ["density"], INVALIDATORS[writer])
    got, counts = run(mode, ["density"], INVALIDATORS[writer])
    assert counts[0] >= 1  # (the case did look ahead before the writer came)
    assert_same_runs(got, want, f"{writer}, lookahead = {mode}")


@pytest.mark.parametrize("mode", ["1", "auto"])
def test_collision_substep_after_a_plain_one(mode):
    from hnanosolver_amd import api

    names = COMBUST + ["collision_sdf"]
    p = api.CombustionParams()

    def script(s, snap):
        s.substep(ITERS, DT, VS, p, False), s.substep(ITERS, DT, VS, p, False), snap()
        made = s.lookahead_counts()
        assert made[0] >= 1
        s.substep(ITERS, DT, VS, p, True), snap()
        assert s.lookahead_counts() == (made[0], made[1])  # the collision substep neither consumed nor produced
        s.substep(ITERS, DT, VS, p, False), snap(), s.substep(ITERS, DT, VS, p, False)

    def script0(s, snap):
        s.substep(ITERS, DT, VS, p, False), s.substep(ITERS, DT, VS, p, False), snap()
        s.substep(ITERS, DT, VS, p, True), snap()
        s.substep(ITERS, DT, VS, p, False), snap(), s.substep(ITERS, DT, VS, p, False)

    want, _ = run("0", names, script0, fuse="0")
    got, _ = run(mode, names, script, fuse="0")
    assert_same_runs(got, want, f"collision after plain, lookahead = {mode}")


def test_auto_policy():
    """auto speculates only after a substep call with the same dt and voxel size: a lone substep and the first one after a change of dt launch the plain kernel"""
    import hnanosolver_amd as H

    H.set_option("lookahead", "auto")
    o, st = start_state(["density"])
    g, s = make_sim(o, ["density"], st, None, VS)
    seen = []
    for dt in (DT, DT, DT, DT / 2, DT / 2, DT / 2, DT):
        s.core_substep(ITERS, dt, VS)
        seen.append(s.lookahead_counts())
    #                 lone     same dt  same dt  new dt   same     same     new dt
    assert seen == [(0, 0), (1, 0), (2, 1), (2, 1), (3, 1), (4, 2), (4, 2)], seen
    s.core_substep(ITERS, DT, VS * 2)  # a new voxel size
    assert s.lookahead_counts() == (4, 2)
    H.set_option("lookahead", "0")
    s.core_substep(ITERS, DT, VS * 2)
    assert s.lookahead_counts() == (4, 2)
    s.close()


def test_captured_substep_never_looks_ahead():
    """under stream capture a substep neither consumes nor produces, and the sim stops looking ahead: a replay writes the velocity unseen.
    (Capturing a substep moves the sim's host-side buffer roles on as running it does, so the graph is replayed exactly once.)"""
    import torch

    import hnanosolver_amd as H

    H.set_option("lookahead", "1")
    o, st = start_state(["density"])
    g, s = make_sim(o, ["density"], st, None, VS)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s.core_substep(ITERS, DT, VS, stream.cuda_stream)
        stream.synchronize()
        assert s.lookahead_counts() == (1, 0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            s.core_substep(ITERS, DT, VS, torch.cuda.current_stream().cuda_stream)
        assert s.lookahead_counts() == (1, 0)
        graph.replay()
    torch.cuda.synchronize()
    s.core_substep(ITERS, DT, VS)
    assert s.lookahead_counts() == (1, 0)  # off for good
    H.set_option("lookahead", "0")
    o2, st2 = start_state(["density"])
    g2, s2 = make_sim(o2, ["density"], st2, None, VS)
    for _ in range(3):
        s2.core_substep(ITERS, DT, VS)
    a, b = download(s, ["density"]), download(s2, ["density"])
    for k in a:
        assert_words(a[k], b[k], f"captured: {k}")
    s.close(), s2.close()
