"""The curl noise of hns_shaping_* without a GPU. (1) hns_shaping_curl_host -- the header the kernel includes, run on the host -- equals the numpy mirror of
tests/shaping_cases.py, written from the text of include/hns.h, in every bit. (2) The mirror's mathematics is held in float64, where a formula that is wrong in kernel and
mirror alike would still show: the analytic gradient against central differences of N, the divergence of the curl by central differences, the curl's continuity across
lattice faces, the table's draw; and the float32 mirror agrees with the float64 restatement to a tolerance derived from the operation count."""
import numpy as np
import pytest

import shaping_cases as sc
from hnanosolver_amd import device

F = np.float32


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))
    assert not len(bad), f"{what}: {len(bad)} voxels differ, first {bad[:4].tolist()}: {a[bad[:4]].tolist()} vs {b[bad[:4]].tolist()}"


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(20)
    leaf = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([rng.integers(-400, 400, (1500, 3)), leaf + [-8, 0, 8], leaf + [-64, -8, 56], [[0, 0, 0], [-1, -1, -1], [7, 8, 9]]]).astype(np.int32)


@pytest.mark.parametrize("octaves", [1, 4])
@pytest.mark.parametrize("frequency", [1.0 / 16, 0.125, 0.9, 1.7])
def test_host_evaluation_equals_the_mirror_in_every_bit(voxels, frequency, octaves):
    """negative coordinates, offsets that put q on both sides of zero, whole leaves (at 0.125 every leaf corner is a lattice point: t = 0), lacunarity 2"""
    for offset in ((0.0, 0.0, 0.0), (-3.25, 0.5, -17.125)):
        spec = sc.spec_of(frequency=frequency, octaves=octaves, lacunarity=2.0, gain=0.5, seed=77, offset=offset)
        want = sc.curl(spec, voxels)
        same_bits(device.shaping_curl_host(spec, voxels), want, f"f {frequency} octaves {octaves} offset {offset}")
        assert np.isfinite(want).all() and (np.abs(want).max(0) > 0.5).all()
    if frequency == 0.125:
        near, I, t = sc.lattice(F(0.125), (0.0, 0.0, 0.0), voxels)
        assert near.all() and ((t == 0).all(1)).sum() >= 3 and (I < 0).any() and (I > 0).any()


def test_seed_gain_and_lacunarity_are_read():
    ijk = np.random.default_rng(3).integers(-50, 50, (200, 3)).astype(np.int32)
    base = sc.spec_of(frequency=0.3, octaves=3, lacunarity=1.5, gain=0.75, seed=1)
    got = {}
    for name, spec in (("base", base), ("seed", {**base, "seed": 2}), ("gain", {**base, "gain": 0.25}), ("lacunarity", {**base, "lacunarity": 2.5}), ("gain 0", {**base, "gain": 0.0})):
        got[name] = sc.curl(spec, ijk)
        same_bits(device.shaping_curl_host(spec, ijk), got[name], name)
    for name in ("seed", "gain", "lacunarity"):
        assert (got[name] != got["base"]).any(1).mean() > 0.9, name
    same_bits(got["gain 0"], sc.curl({**base, "octaves": 1}, ijk), "gain 0 leaves octave 0 (the others add +0)")


def test_the_far_rule():
    """|q| >= 4194304 in any component: the octave contributes exactly +0; just inside it still evaluates. With lacunarity 2 the second octave of a voxel at 2^21 is far"""
    edge = 4194304
    ijk = np.array([[edge, 0, 0], [edge - 1, 3, 5], [-edge, 1, 1], [-edge + 1, 1, 1], [5, edge, 7], [5, 7, -edge], [2 ** 31 - 1, 0, 0], [-(2 ** 31), 0, 0], [edge // 2, 1, 2], [edge // 2 - 1, 1, 2]], np.int32)
    one = sc.spec_of(frequency=1.0, octaves=1, seed=4, offset=(0.0, 0.0, 0.0))
    want = sc.curl(one, ijk)
    same_bits(device.shaping_curl_host(one, ijk), want, "far rule, one octave")
    far = np.array([1, 0, 1, 0, 1, 1, 1, 1, 0, 0], bool)
    assert (want[far].view(np.uint32) == 0).all(), "a far voxel is not exactly +0"
    assert (want[~far] != 0).any(1).all(), "a voxel just inside the rule did not evaluate"
    two = {**one, "octaves": 2, "lacunarity": 2.0, "gain": 0.5}
    want2 = sc.curl(two, ijk)
    same_bits(device.shaping_curl_host(two, ijk), want2, "far rule, two octaves")
    same_bits(want2[:9], want[:9], "an octave beyond the rule adds +0")  # (voxel 8: 2 * 2^21 is the rule's edge)
    assert (want2[9] != want[9]).any(), "the second octave of a voxel just inside the rule did not evaluate"
    # an offset carries a voxel over the rule, and an overflowing f_o is far everywhere
    moved = {**one, "offset": (4194300.0, 0.0, 0.0)}
    want3 = sc.curl(moved, np.array([[3, 0, 0], [4, 0, 0]], np.int32))
    same_bits(device.shaping_curl_host(moved, [[3, 0, 0], [4, 0, 0]]), want3, "offset")
    assert (want3[0] != 0).any() and (want3[1].view(np.uint32) == 0).all()
    big = sc.spec_of(frequency=3e38, octaves=2, lacunarity=10.0, seed=1)
    ijk3 = np.array([[0, 0, 0], [1, 1, 1], [0, 5, 0]], np.int32)
    same_bits(device.shaping_curl_host(big, ijk3), sc.curl(big, ijk3), "overflowing frequency")


def test_the_table_is_drawn_uniformly():
    rng = np.random.default_rng(8)
    s = sc.octave_constants(sc.spec_of(seed=123))[0][2]
    I = rng.integers(-1000, 1000, (40000, 3)).astype(np.int32)
    with np.errstate(over="ignore"):
        h = sc.H(sc.H(sc.H(s ^ I[:, 0].astype(np.uint32)) ^ I[:, 1].astype(np.uint32)) ^ I[:, 2].astype(np.uint32))
    for m in range(3):
        counts = np.bincount((h >> np.uint32(4 * m)) & np.uint32(15), minlength=16)
        assert np.abs(counts - 2500).max() < 5 * np.sqrt(2500 * 15 / 16), counts  # five standard deviations of a uniform draw
    assert (sc.TABLE != 0).sum(1).tolist() == [2] * 16 and not np.signbit(sc.TABLE[sc.TABLE == 0]).any()


# ---------------------------------------------------------------------------------------------------------------
# the mathematics, in float64
# ---------------------------------------------------------------------------------------------------------------


def at(q):
    """cells and fractions of continuous lattice positions q [n, 3] (float64)"""
    I = np.floor(q).astype(np.int32)
    return I, q - I


def positions(n, seed):
    """lattice positions at least 0.02 from every lattice plane"""
    rng = np.random.default_rng(seed)
    return rng.integers(-20, 20, (n, 3)) + rng.uniform(0.02, 0.98, (n, 3))


S = sc.octave_constants(sc.spec_of(seed=2024))[0][2]


def N64(q):
    return sc.potential(*at(q), S)


def curl64(q):
    return sc.cell_curl(*at(q), S, T=np.float64)


def test_the_analytic_gradient_and_the_divergence_of_the_curl_converge_at_second_order():
    """central differences at steps 1e-2, 5e-3, 2.5e-3: the error of the analytic gradient against them, and the central-difference divergence of the curl, each fall to
    at most 0.3 of the previous one (theory: 0.25; rounding is eight orders of magnitude below these errors)"""
    q = positions(400, 1)
    q = q[(np.minimum(q - np.floor(q), np.ceil(q) - q) > 0.021).all(1)]  # (a step of 1e-2 stays inside the cell)
    grad = sc.cell_curl(*at(q), S, T=np.float64, gradient=True)  # [n, channel, axis]
    g_err, d_err = [], []
    for step in (1e-2, 5e-3, 2.5e-3):
        fd = np.empty_like(grad)
        div = np.zeros(len(q))
        for axis in range(3):
            e = np.zeros(3)
            e[axis] = step
            fd[:, :, axis] = (N64(q + e) - N64(q - e)) / (2 * step)
            div += (curl64(q + e)[:, axis] - curl64(q - e)[:, axis]) / (2 * step)
        g_err.append(np.abs(fd - grad).max())
        d_err.append(np.abs(div).max())
    print(f"gradient error {g_err}, ratios {g_err[1] / g_err[0]:.4f} {g_err[2] / g_err[1]:.4f}; divergence {d_err}, ratios {d_err[1] / d_err[0]:.4f} {d_err[2] / d_err[1]:.4f}")
    assert g_err[0] > 1e-6 and d_err[0] > 1e-6  # (there is an error to converge)
    for errs in (g_err, d_err):
        assert errs[1] <= 0.3 * errs[0] and errs[2] <= 0.3 * errs[1], errs


def test_the_curl_is_continuous_across_lattice_faces():
    rng = np.random.default_rng(5)
    worst = 0.0
    for axis in range(3):
        q = rng.integers(-20, 20, (300, 3)) + rng.uniform(0.02, 0.98, (300, 3))
        q[:, axis] = np.round(q[:, axis])
        lo, hi = q.copy(), q.copy()
        lo[:, axis] -= 1e-9
        hi[:, axis] += 1e-9
        assert (np.floor(lo[:, axis]) != np.floor(hi[:, axis])).all()
        worst = max(worst, np.abs(curl64(hi) - curl64(lo)).max())
    print(f"largest jump of the curl across a lattice face at +-1e-9: {worst:.3e}")
    assert worst <= 1e-6


def test_the_float32_mirror_agrees_with_the_float64_restatement():
    """Tolerance from the operation count. A curl component is the difference of two partials; a partial is (slope * nest of 4 differences) + nest of 8 gradients. Every
    rounded float32 operation adds at most eps/2 of its result, which is at most M, the largest magnitude among the partials' inputs and results; such an error then passes
    through lerps (convex: no growth), at most one difference (x 2) and the multiply by the slope (<= 1.875), so it reaches the result grown at most 3.75-fold. The
    operations that feed one component: 2 partials x [8 corners x (3 p + 3 multiplies + 2 adds) shared among them, 2 x 7 fades + 6 slope, 4 differences, 3 lerps x 3,
    1 multiply, 7 lerps x 3, 1 add] + 1 = 2 x (64 + 20 + 4 + 9 + 1 + 21 + 1) + 1 = 241. The fraction itself is exact away from the lattice planes."""
    q32 = positions(4000, 9).astype(F)
    I = np.floor(q32).astype(np.int32)
    t32 = q32 - I.astype(F)
    got = sc.cell_curl(I, t32, S)
    want = sc.cell_curl(I, t32.astype(np.float64), S, T=np.float64)
    grad = sc.cell_curl(I, t32.astype(np.float64), S, T=np.float64, gradient=True)
    M = max(np.abs(grad).max(), 2.0)  # (2: |p| < 1 and |g| <= 1 give |d| < 2; the differences of d are below 4 but enter through the slope's factor above)
    tol = 241 * 3.75 * (np.finfo(F).eps / 2) * M
    err = np.abs(got - want).max()
    norm = np.linalg.norm(want, axis=1)
    print(f"float32 mirror against float64: largest difference {err:.3e}, derived tolerance {tol:.3e} (M = {M:.3f}); one octave over {len(q32)} samples: "
          f"|c| mean {norm.mean():.3f}, largest component {np.abs(want).max():.3f}, mean |component| {np.abs(want).mean():.3f}")
    assert err <= tol
    assert 0.5 < np.abs(want).mean() < 1.2 and 3.0 < np.abs(want).max() < 4.5  # what include/hns.h tells users to choose an amplitude by
