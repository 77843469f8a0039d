"""Signed zeros, subnormals, NaN, inf, overflow and threshold values through every HIP kernel, on the GPU.

The comparator is the device-semantics build of the oracle (oracle/liboracle_dev.so: symmetric min/max with -0 < +0, saturating
float -> int): same_bits, zero signs included, a NaN equal to any NaN. Where the reference's own kernel
bodies travelled (oracle/_ref/libhns_refk.so, a host build), the HIP results may differ from them in the sign of a zero only, and
in exactly the words in which the device-semantics oracle differs from the stock oracle. The conditions of
special_cases.check_comparator are asserted on the comparator's output in every case; no case is filtered after the fact."""
import numpy as np
import pytest

import special_cases as sc
from hip_kernels import HipKernels
from oracle_lib import OracleGrid, RefKernelGrid, oracle_device, reference_kernels, reference_samplers

pytestmark = pytest.mark.gpu

HAVE_REF = reference_kernels() is not None and reference_samplers() is not None


def compare(o, w, sor_iters):
    """every kernel, collision off and on: HIP == device-semantics oracle; HIP vs the reference's kernels = stock vs device oracle"""
    H, D = HipKernels(o, sc.VS), OracleGrid(o, lib=oracle_device())
    for coll in (False, True):
        want = sc.run_kernels(D, w, coll, sor_iters)
        sc.check_comparator(w, want)
        if w.cls == "nonfinite" and w.planted["fields"] and not coll:
            assert sc.limiter_swallowed_a_nan(w, want["advect_scalar"]) >= 1
        got = sc.run_kernels(H, w, coll, sor_iters)
        bad = {n: sc.describe(got[n], want[n]) for n in want if not sc.same_bits(got[n], want[n])}
        assert not bad, f"coll={coll}: " + "; ".join(f"{n}: {d}" for n, d in bad.items())
        if HAVE_REF:
            ref, stock = sc.run_kernels(RefKernelGrid(o), w, coll, sor_iters), sc.run_kernels(OracleGrid(o), w, coll, sor_iters)
            for n in want:
                ok, at = sc.same_but_zero_sign(got[n], ref[n])
                assert ok, f"{n} coll={coll} vs the reference's kernels: {sc.describe(got[n], ref[n])}"
                ok2, at2 = sc.same_but_zero_sign(want[n], stock[n])
                assert ok2 and np.array_equal(at, at2), f"{n} coll={coll}: zero signs differ from the reference's in {len(at)} words, predicted {len(at2)}"


@pytest.mark.parametrize("where", sc.WHERE)
@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("leaves", list(sc.LEAF_SETS))
def test_hip_kernels_equal_device_oracle(leaves, cls, where):
    o = sc.LEAF_SETS[leaves]()
    # 7 iterations spread a NaN over a ball of radius 14: in `nonfinite` that case runs on 110k voxels (below)
    compare(o, sc.Workload(o, cls, where), (1, 2, 3, 4) if cls == "nonfinite" else (1, 2, 3, 4, 7))


@pytest.mark.parametrize("leaves", ["ragged32", "ragged32_off_origin", "sparse_far"])
@pytest.mark.parametrize("cls", ["zeros", "nonfinite"])
def test_long_back_traces_through_the_origin_hash(leaves, cls):
    o = sc.LEAF_SETS[leaves]()
    compare(o, sc.Workload(o, cls, "both", seed=1, speed=30.0), (1, 4))


def test_seven_iterations_with_one_nan_on_110k_voxels():
    o = sc.LEAF_SETS_BIG["dense48"]()
    n = len(o) * 512
    rng = np.random.default_rng(8)
    div, p0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    p0[(len(o) // 2) * 512 + 77] = np.nan
    want = OracleGrid(o, lib=oracle_device()).rbgs_iterations(div, float(np.float32(sc.VS)), sc.OMEGA, 7, p0)
    assert 0 < np.isnan(want).mean() <= 0.5
    got = HipKernels(o, sc.VS).rbgs_iterations(div, float(np.float32(sc.VS)), sc.OMEGA, 7, p0)
    assert sc.same_bits(got, want), sc.describe(got, want)


@pytest.mark.parametrize("collision", [False, True])
@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("leaves", ["ragged32", "dense32"])
def test_hip_operators_equal_device_oracle(leaves, cls, collision):
    """Compute_Sim (vorticity on, 7 iterations) and ProjectNonDivergent through the drop-in operators"""
    from hnanosolver_amd import api

    o = sc.LEAF_SETS[leaves]()
    p = api.CombustionParams(factorScale=1.0, vorticityScale=0.4)
    want = sc.run_operators(OracleGrid(o, lib=oracle_device()), o, cls, collision, p)
    got = sc.run_operators(HipKernels(o, sc.VS), o, cls, collision, p)
    for n in want:
        assert np.isnan(want[n]).mean() <= 0.5, n
        assert sc.same_bits(got[n], want[n]), f"{n}: {sc.describe(got[n], want[n])}"


@pytest.mark.parametrize("p", [1, 9])
def test_substeps_on_the_state_a_regrid_leaves(p):
    """A regrid fills its new leaves with +0 and collision_sdf with the byte fill 0x01010101 = 2.37e-38: three substeps with collision
    on from that state, against a fresh sim of the same state and against the device-semantics oracle's compute_sim."""
    from frame_cases import COMBUST, assert_same, download, make_sim
    from hnanosolver_amd import api, fields

    R = 16
    o = fields.dense_leaves(R)
    names = COMBUST + ["collision_sdf"]
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + COMBUST}
    st["collision_sdf"] = fields.sphere_sdf(o, R, center=(0.4, 0.5, 0.5), radius=0.2)
    g, s = make_sim(o, names, st, None, 1.0 / R)
    s.substep(3, sc.DT, 1.0 / R, api.CombustionParams(), True)
    s.regrid(p)
    dom = np.ascontiguousarray(s.grid.coords()[::512])
    assert len(dom) > len(o)
    state = download(s, names)
    new = np.repeat(~(dom[:, None, :] == o[None, :, :]).all(2).any(1), 512)
    assert new.any() and (state["collision_sdf"][new] == sc.SDF_FILL).all() and all((state[n][new].view(np.uint32) == 0).all() for n in COMBUST)
    g2, s2 = make_sim(dom, names, state, None, 1.0 / R)
    D = OracleGrid(dom, lib=oracle_device())
    want = {k: v.copy() for k, v in state.items()}
    params = api.CombustionParams(factorScale=1.0, vorticityScale=0.4)
    for _ in range(3):
        s.substep(7, sc.DT, 1.0 / R, params, True)
        s2.substep(7, sc.DT, 1.0 / R, params, True)
        cur = {n: want[n] for n in names}
        sdf = want["collision_sdf"].copy()
        assert D.compute_sim(want["vel"], cur, 7, sc.DT, 1.0 / R, params, True) == 0
        want["collision_sdf"][...] = sdf  # Compute hands it back zeroed; a device-resident sim keeps it
    got = download(s, names)
    assert_same(got, download(s2, names), f"p={p}: regridded sim vs a fresh sim of the same state")
    for n in ["vel"] + COMBUST:
        assert np.isnan(want[n]).mean() <= 0.5
        assert sc.same_bits(got[n], want[n]), f"p={p} {n}: {sc.describe(got[n], want[n])}"
    s.close(), s2.close()
