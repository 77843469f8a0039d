"""Signed zeros, subnormals, NaN, inf, overflow and threshold values through every kernel -- the part that runs without a GPU.

1. the stock oracle against the reference's own kernel bodies (oracle/_ref/libhns_refk.so) on the input classes of
   tests/special_cases.py: same_bits (a NaN equals any NaN), so that the oracle stays a valid comparator on such inputs;
2. the device-semantics build of the oracle (oracle/liboracle_dev.so: the GPU's symmetric min/max and saturating float -> int
   conversion) against the stock build: it may differ in the sign of a zero, in the three advection
   kernels only, and in the `zeros` class it must;
3. (closed-form cases for what neither library can vouch for: tests/kats.py SPECIAL_CASES, run by tests/test_kats.py.)
The conditions of special_cases.check_comparator are asserted on the comparator's output in every case."""
import numpy as np
import pytest

import special_cases as sc
from hnanosolver_amd import api
from oracle_lib import OracleGrid, RefKernelGrid, oracle_device, reference_kernels, reference_samplers

needs_ref = pytest.mark.skipif(reference_kernels() is None or reference_samplers() is None,
                               reason="oracle/_ref/libhns_refk.so not available (needs the reference checkout + the image's CUDA headers to build)")
PARAMS = dict(factorScale=1.0, vorticityScale=0.4)


def test_the_classes_are_what_they_say():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(1 << 16).astype(np.float32)
    z = sc.plant("zeros", a, rng)
    assert 0.55 < (z == 0).mean() < 0.65 and 0.4 < np.signbit(z[z == 0]).mean() < 0.6
    s = sc.plant("subnormal", a, rng)
    assert sc.is_subnormal(s).mean() > 0.3 and (s == sc.SDF_FILL).any() and (s == sc.FLT_MIN).any() and (s == sc.SUB_MAX).any()
    with np.errstate(over="ignore", invalid="ignore"):
        h = sc.plant("huge", a, rng)
        assert np.isfinite(h).all() and np.isinf(h * h).any()
    n = sc.plant("nonfinite", a, rng)
    assert np.isnan(n).any() and np.signbit(n[np.isnan(n)]).any() and not np.signbit(n[np.isnan(n)]).all() and (n == np.inf).any() and (n == -np.inf).any()
    assert ((n.view(np.uint32) & 0x7FC00000) == 0x7FC00000)[np.isnan(n)].all()  # quiet
    o = sc.LEAF_SETS["ragged32_off_origin"]()
    assert len(o) == 32 and (np.maximum(o, -(o + 7)).max(axis=1) > 64).all()  # Chebyshev distance of every leaf from (0, 0, 0)
    assert (sc.LEAF_SETS["ragged32"]() == 0).all(1).any()
    # threshold velocities: positions exactly on integers, on leaf faces, and within an ulp of them
    from hnanosolver_amd import fields

    o = sc.LEAF_SETS["ragged32"]()
    v = sc.threshold_velocity(np.zeros((len(o) * 512, 3), np.float32) + np.float32(0.3), o, rng)
    pos = fields.leaves_to_coords(o).astype(np.float32) - np.float32(sc.SDT) * v
    frac = pos - np.floor(pos)
    assert (frac[v != np.float32(0.3)] == 0).mean() > 0.2 and ((frac > 0) & ((frac < 1e-5) | (frac > 1 - 1e-5))).sum() > 100
    a, b = np.array([0.0, -0.0, np.nan, 1.0], np.float32), np.array([-0.0, -0.0, -np.nan, 1.0], np.float32)
    assert not sc.same_bits(a, b) and sc.same_but_zero_sign(a, b) == (True, [0]) and sc.same_bits(a[1:], b[1:])
    assert not sc.same_but_zero_sign(a, np.array([0.0, 0.0, 1.0, 1.0], np.float32))[0]


# ---------------------------------------------------------------------------------------------------------------
# 1. stock oracle == the reference's kernel bodies
# ---------------------------------------------------------------------------------------------------------------


@needs_ref
@pytest.mark.parametrize("where", sc.WHERE)
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_oracle_equals_reference_kernels(cls, where):
    o = sc.LEAF_SETS["ragged32"]()
    O, K = OracleGrid(o), RefKernelGrid(o)
    w = sc.Workload(o, cls, where)
    for coll in (False, True):
        want, got = sc.run_kernels(K, w, coll), sc.run_kernels(O, w, coll)
        sc.check_comparator(w, want)
        for name in want:
            assert sc.same_bits(got[name], want[name]), f"{name} coll={coll}: {sc.describe(got[name], want[name])}"
        if cls == "nonfinite" and where != "velocity" and not coll:
            assert sc.limiter_swallowed_a_nan(w, want["advect_scalar"]) >= 1


@needs_ref
@pytest.mark.parametrize("collision", [False, True])
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_oracle_drivers_equal_reference_launch_sequences(cls, collision):
    o = sc.LEAF_SETS["ragged32"]()
    p = api.CombustionParams(**PARAMS)
    want, got = sc.run_operators(RefKernelGrid(o), o, cls, collision, p), sc.run_operators(OracleGrid(o), o, cls, collision, p)
    for name in want:
        assert np.isnan(want[name]).mean() <= 0.5, name
        assert sc.same_bits(got[name], want[name]), f"{name}: {sc.describe(got[name], want[name])}"


# ---------------------------------------------------------------------------------------------------------------
# 2. device semantics vs stock: the sign of a zero, in advection only
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("leaves", ["ragged32", "ragged32_off_origin"])
@pytest.mark.parametrize("where", sc.WHERE)
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_device_semantics_differ_in_zero_sign_of_advection_only(cls, where, leaves):
    o = sc.LEAF_SETS[leaves]()
    S, D = OracleGrid(o), OracleGrid(o, lib=oracle_device())
    assert S.L.orc_device_semantics() == 0 and D.L.orc_device_semantics() == 1
    w = sc.Workload(o, cls, where)
    flipped = 0
    for coll in (False, True):
        stock, dev = sc.run_kernels(S, w, coll), sc.run_kernels(D, w, coll)
        sc.check_comparator(w, dev)
        for name in stock:
            ok, at = sc.same_but_zero_sign(dev[name], stock[name])
            assert ok, f"{name} coll={coll}: more than a zero's sign: {sc.describe(dev[name], stock[name])}"
            if sc.KERNEL_OF[name] in sc.ADVECTION:
                flipped += len(at)
            else:
                assert len(at) == 0, f"{name} coll={coll}: {len(at)} zero signs differ outside advection"
    if cls == "zeros":
        assert flipped >= 1, "the device-semantics switch changed nothing: is it switched?"


@pytest.mark.parametrize("collision", [False, True])
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_device_semantics_whole_substep(cls, collision):
    """Compute_Sim derives everything from advected values: zero signs may differ anywhere in it, nothing else may.
    ProjectNonDivergent has no min/max and no conversion in it: not a bit."""
    o = sc.LEAF_SETS["ragged32"]()
    p = api.CombustionParams(**PARAMS)
    stock, dev = sc.run_operators(OracleGrid(o), o, cls, collision, p), sc.run_operators(OracleGrid(o, lib=oracle_device()), o, cls, collision, p)
    for name in stock:
        assert np.isnan(dev[name]).mean() <= 0.5, name
        ok, at = sc.same_but_zero_sign(dev[name], stock[name])
        assert ok, f"{name}: {sc.describe(dev[name], stock[name])}"
        if name == "projected":
            assert len(at) == 0
