"""Diffusing a sim without a GPU: the host constants of hns_diffusion_schedule_host equal the numpy mirror's (tests/diffusion_cases.py) in every byte, and the mirror --
the header's text in numpy, which the kernels must equal word for word on the MI355X (tests/test_diffusion_gpu.py) -- is held to the mathematics it claims:

  * in float64 against its own 20,000-iteration Jacobi limit (an iterate that equals its predecessor, or the one before it, in every bit fixes every later one, so
    the run ends there with the 20,000th iterate exactly):
    Jacobi's max error after k iterations is <= 2 rho^k max|b| (x^0 = b and the solution both lie in [min b, max b], and the iteration contracts the max norm by
    rho: |x^k - x| <= rho^k |b - x| <= rho^k (max b - min b)); Chebyshev's is <= 2 sqrt(n) (2 sigma^k / (1 + sigma^2k)) max|b| (the Chebyshev polynomial bounds the
    2-norm of the error by that factor times |b - x|_2 <= sqrt(n) |b - x|_max, and the max norm is below the 2-norm). Both are derived, not measured;
  * in float32 against float64 at the same iteration count: <= 16 * 2^-24 * max|b| / (1 - rho) -- an iteration commits at most eight roundings of 2^-24 relative on values
    no larger than max|b| (Chebyshev: within a small multiple of it), twice that for slack, and errors of earlier iterations are contracted by rho, a geometric sum;
  * every Jacobi iterate of a float field within [min b, max b]; the limit conserves the sum of a float field and, with walls, not the velocity's; voxels that are no
    unknowns keep their bytes.

Measured here (printed by the tests), max|b| = 8: at a = 4 after 40 iterations the error against the limit is 3.2e-2 for Jacobi and 1.4e-4 for Chebyshev (bounds 3.1
and 3.0e-2); at a = 0.05 after 8 iterations 1.0e-6 and 8.6e-8, float32's resolution; float32 against float64 at most 1.1e-5 (a = 32, Chebyshev, 8 iterations; bound
1.6e-3), elsewhere below 2.3e-6."""
import functools
import math

import numpy as np
import pytest

import diffusion_cases as dc
from hnanosolver_amd import device

F, D = np.float32, np.float64
A_VALUES = (0.05, 0.5, 4.0, 32.0)


@pytest.mark.parametrize("iterations", [1, 2, 3, 256])
@pytest.mark.parametrize("a", [0.0, 1e-40, 1e-30, 0.05, 0.5, 4.0, 32.0, 2.0 ** 20])
def test_schedule_host_equals_the_mirror_in_every_byte(a, iterations):
    for coefficient, dt, vs in ((a, 1.0, 1.0), (a * 0.37, 0.04, 1.0 / 32)):
        got, want = device.diffusion_schedule_host(coefficient, dt, vs, iterations), dc.schedule(coefficient, dt, vs, iterations, F)
        for k in ("a", "rho", "r", "omega"):
            assert np.asarray(got[k], F).tobytes() == np.asarray(want[k], F).tobytes(), (k, got[k], want[k])
        assert got["omega"][0] == 1 and (got["omega"][iterations:] == 0).all() and (got["omega"][:iterations] >= 1).all()
        assert got["r"][0] == 1 and (np.diff(got["r"]) <= 0).all()


def start_fields():
    n = len(dc.fixture()["origins"]) * 512
    rng = np.random.default_rng(17)
    vel = rng.standard_normal((n, 3)).astype(F)
    return {"b": (rng.standard_normal(n) * 2 + 1).astype(F), "vel": vel, "speed": np.abs(vel)}  # (speed: a velocity of one sign)


@functools.lru_cache(maxsize=None)
def geometry(collide):
    fx = dc.fixture()
    n = len(fx["origins"]) * 512
    unknown, solid = dc.classes(n, fx["active"], fx["sdf"], collide, 0.0)
    open_, wall = dc.faces(fx["nb"], unknown, solid)
    return unknown, open_, wall


def run(field, a, iterations, method, dtype, collide=False, every=None):
    unknown, open_, wall = geometry(collide)
    count = open_.sum(0) + (0 if field == "b" else wall.sum(0))
    return dc.iterate(start_fields()[field], dc.fixture()["nb"], open_, count, unknown, dc.schedule(a, 1.0, 1.0, iterations, dtype), iterations, dc.METHODS[method], dtype, every)


class Converged(Exception):
    pass


@functools.lru_cache(maxsize=None)
def limit(field, a, collide):
    """the 20,000th Jacobi iterate in float64. An iterate that equals its predecessor in every bit is every later one; one that equals the one before its predecessor
    (the last bit of some voxels flips to and fro) repeats with period two, and the 20,000th is the one of even index. Either ends the run: the result is exact."""
    seen = {}

    def every(k, x):
        seen[k] = x
        seen.pop(k - 3, None)
        if k >= 3 and (x.tobytes() == seen[k - 1].tobytes() or x.tobytes() == seen[k - 2].tobytes()):
            raise Converged

    try:
        run(field, a, 20000, "jacobi", D, collide, every)
    except Converged:
        pass
    k = max(seen)
    return seen[k if k % 2 == 0 else k - 1]


@pytest.mark.parametrize("a, iterations", [(4.0, 40), (0.05, 8)])
def test_float64_iterates_approach_the_limit_within_the_derived_bounds(a, iterations):
    unknown = geometry(False)[0]
    x, b = limit("b", a, False), start_fields()["b"].astype(D)
    top, n = np.abs(b[unknown]).max(), int(unknown.sum())
    rho = 6 * a / (1 + 6 * a)
    sigma = rho / (1 + math.sqrt(1 - rho * rho))
    for method, bound in (("jacobi", lambda k: 2 * rho ** k * top), ("chebyshev", lambda k: 2 * math.sqrt(n) * (2 * sigma ** k / (1 + sigma ** (2 * k))) * top)):
        errors = {}
        run("b", a, iterations, method, D, every=lambda k, xk: errors.__setitem__(k, np.abs(xk - x)[unknown].max()))
        print(f"a = {a} {method}: error after {iterations} iterations {errors[iterations]:.3g} (bound {bound(iterations):.3g}); after 1: {errors[1]:.3g} ({bound(1):.3g})")
        for k, e in errors.items():
            assert e <= bound(k), (method, k, e, bound(k))
    assert np.array_equal(x[~unknown], b[~unknown])


@pytest.mark.parametrize("method", sorted(dc.METHODS))
@pytest.mark.parametrize("a", A_VALUES)
def test_float32_mirror_stays_within_rounding_of_the_float64_one(a, method):
    rho = 6 * a / (1 + 6 * a)
    for field, collide in (("b", False), ("vel", True)):
        unknown = geometry(collide)[0]
        top = np.abs(start_fields()[field][unknown]).max()
        bound = 16 * 2.0 ** -24 * top / (1 - rho)
        for iterations in (3, 8, 40):
            x32, x64 = run(field, a, iterations, method, F, collide), run(field, a, iterations, method, D, collide)
            assert x32.dtype == F and x64.dtype == D
            err = np.abs(x32.astype(D) - x64)[unknown].max()
            print(f"a = {a} {method} {field} k = {iterations}: float32 against float64 {err:.3g} (bound {bound:.3g})")
            assert err <= bound, (field, iterations, err, bound)


@pytest.mark.parametrize("a", A_VALUES)
def test_every_jacobi_iterate_of_a_float_field_lies_between_the_ends_of_b(a):
    unknown = geometry(True)[0]
    b = start_fields()["b"]
    lo, hi = b[unknown].min(), b[unknown].max()
    slack = 4 * np.spacing(np.abs(b[unknown]).max())

    def every(k, x):
        assert x[unknown].min() >= lo - slack and x[unknown].max() <= hi + slack, k

    run("b", a, 40, "jacobi", F, True, every)


def test_the_limit_conserves_a_float_field_and_walls_take_the_velocitys_momentum():
    a = 4.0
    for collide in (False, True):
        unknown = geometry(collide)[0]
        b, x = start_fields()["b"].astype(D), limit("b", a, collide)
        assert abs(x[unknown].sum() - b[unknown].sum()) <= 1e-9 * np.abs(b[unknown]).sum(), collide
    # a velocity of one sign: every wall face takes momentum, so the sum falls by far more than any rounding; without walls it is conserved like a float field
    v = start_fields()["speed"].astype(D)
    unknown, _, wall = geometry(True)
    assert wall.any()
    x = limit("speed", a, True)
    lost = 1 - x[unknown].sum() / v[unknown].sum()
    print(f"the velocity's sum over the unknowns falls by {lost:.3g} of itself")
    assert lost > 1e-3
    unknown0 = geometry(False)[0]
    assert abs(limit("speed", a, False)[unknown0].sum() - v[unknown0].sum()) <= 1e-9 * v[unknown0].sum()


@pytest.mark.parametrize("method", sorted(dc.METHODS))
def test_voxels_that_are_no_unknowns_keep_their_bytes_and_a_zero_a_skips_the_term(method):
    fx = dc.fixture()
    n = len(fx["origins"]) * 512
    rng = np.random.default_rng(23)
    state = {"vel": rng.standard_normal((n, 3)).astype(F), "density": rng.standard_normal(n).astype(F), "heat": rng.standard_normal(n).astype(F),
             "collision_sdf": np.array(fx["sdf"])}
    out = dc.apply_mirror(fx["origins"], state, 0.04, 1.0 / 32, {"density": 0.01, "heat": 0.0}, viscosity=0.02, iterations=5, method=method, collide=True, threshold=0.0,
                          active=fx["active"])
    unknown = geometry(True)[0]
    assert out["heat"] is state["heat"] and out["collision_sdf"] is state["collision_sdf"]
    for k in ("vel", "density"):
        changed = (out[k].view(np.uint32) != state[k].view(np.uint32)).reshape(n, -1).any(1)
        assert not changed[~unknown].any() and changed[unknown].mean() > 0.9, k
    same = dc.apply_mirror(fx["origins"], state, 0.0, 1.0 / 32, {"density": 0.01}, viscosity=0.02, iterations=5, method=method)
    assert same["vel"] is state["vel"] and same["density"] is state["density"]
