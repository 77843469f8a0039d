"""TEST HELPER: the special-value input classes, the leaf sets they are planted on, the two equalities and the conditions a
comparison must keep -- stated once for tests/test_special_values.py (CPU), tests/test_special_values_gpu.py and the
special-value cases of the variant / blocked-SOR / multi-GPU tests.

Input classes (each deterministic from the generator it is given, each applicable to any float32 array):

  zeros       60 % of the values replaced by zero, sign at random
  subnormal   half the values times 1e-38, a tenth of them times a further 1e-5; a few exact FLT_MIN, 0x01010101 (the byte
              fill a regrid gives collision_sdf), the largest subnormal
  huge        2 % of the values times 3e37: products overflow to inf, inf - inf occurs
  nonfinite   quiet NaN of both signs, +inf, -inf planted at `rate` each (no signalling NaN: no kernel or upload makes one)
  thresholds  values exactly at and one ulp either side of the constants the kernels compare with (THRESHOLD_VALUES); for the
              velocity, back-traced positions exactly on a cell boundary, a leaf boundary and the two positions where the
              LDS-box test "cell - (leaf origin - 1) in [0, 8]" flips, and one ulp either side of each (threshold_velocity)

Equalities:
  same_bits(a, b)            equal as 32-bit words, except that a NaN equals any NaN
  same_but_zero_sign(a, b)   as above, and +0 equals -0; returns the positions where only the sign of a zero differs
"""
from __future__ import annotations

import numpy as np

from hnanosolver_amd import fields

F = np.float32
CLASSES = ("zeros", "subnormal", "huge", "nonfinite", "thresholds")
WHERE = ("fields", "velocity", "both")
FLT_MIN = np.frombuffer(np.uint32(0x00800000).tobytes(), F)[0]
SDF_FILL = np.frombuffer(np.uint32(0x01010101).tobytes(), F)[0]  # 2.37e-38
SUB_MAX = np.frombuffer(np.uint32(0x007FFFFF).tobytes(), F)[0]
QNAN = (np.frombuffer(np.uint32(0x7FC00000).tobytes(), F)[0], np.frombuffer(np.uint32(0xFFC00000).tobytes(), F)[0])

# the solver's parameters in every special-value case: scaled_dt = dt / voxel_size = 2 exactly, so that a velocity of d / 2
# back-traces by exactly d voxels
DT, VS = 1.0 / 16.0, 1.0 / 32.0
INV = 32.0
SDT = 2.0
AMBIENT, STRENGTH = 23.0, 1.5
OMEGA = 1.93


def _around(x):
    x = F(x)
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


# 0 (sdf < 0, oxygen < 0, fmaxf(0, .)), the collision blend margin 0.1f (Kernel.cu:90,441,817), the blend divisor 1.5f (:443),
# the fuel threshold 0.001f (:940), temperature == ambient (:840), flame's fminf(1, burn * 10) (:963), the normal's 1e-6f (:45)
THRESHOLD_VALUES = np.array(
    [F(0.0), F(-0.0), np.nextafter(F(0), F(1)), np.nextafter(F(0), F(-1))]
    + _around(0.1) + _around(1.5) + _around(0.001) + _around(AMBIENT) + _around(1.0) + _around(1e-6) + _around(0.5) + _around(0.25),
    dtype=F)


def plant(cls: str, a: np.ndarray, rng, rate: float = 0.003, huge_share: float = 0.02) -> np.ndarray:
    """a copy of float32 array `a` with class `cls` planted"""
    v = np.array(a, dtype=F)
    f = v.reshape(-1)
    n = f.size
    if cls == "zeros":
        m = rng.random(n) < 0.6
        f[m] = np.where(rng.random(int(m.sum())) < 0.5, F(0.0), F(-0.0))
    elif cls == "subnormal":
        m = rng.random(n) < 0.5
        f[m] *= F(1e-38)
        m2 = m & (rng.random(n) < 0.2)  # a tenth of all values
        f[m2] *= F(1e-5)
        for sv in (FLT_MIN, SDF_FILL, SUB_MAX, -SUB_MAX):
            f[rng.integers(0, n, size=max(1, n // 2048))] = sv
    elif cls == "huge":
        m = rng.random(n) < huge_share
        with np.errstate(over="ignore"):
            f[m] *= F(3e37)
    elif cls == "nonfinite":
        for sv in (QNAN[0], QNAN[1], F(np.inf), F(-np.inf)):
            k = max(1, int(round(rate * n * (0.5 if sv != sv else 1.0))))  # NaN of both signs: `rate` together
            f[rng.choice(n, size=min(k, n), replace=False)] = sv
    elif cls == "thresholds":
        m = np.flatnonzero(rng.random(n) < 0.3)
        f[m] = THRESHOLD_VALUES[rng.integers(0, len(THRESHOLD_VALUES), size=len(m))]
    else:
        raise KeyError(cls)
    return v


def plant_few(a: np.ndarray, rng, count: int) -> np.ndarray:
    """`count` non-finite values (NaN first, then +inf, -inf, -NaN) at distinct places: the red-black solve multiplies a NaN's
    reach by the iteration count, so its inputs take a stated number of plantings, not a rate"""
    v = np.array(a, dtype=F)
    f = v.reshape(-1)
    where = rng.choice(f.size, size=count, replace=False)
    for w, sv in zip(where, (QNAN[0], F(np.inf), F(-np.inf), QNAN[1])):
        f[w] = sv
    return v


def threshold_velocity(vel: np.ndarray, origins: np.ndarray, rng) -> np.ndarray:
    """For 30 % of the voxels one velocity component is replaced so that the back-traced position c - SDT * v of that axis is,
    with leaf origin o and local coordinate l = c - o: a cell boundary (an integer displacement), the leaf's faces o and o + 8,
    or o - 1 / o + 8, where the cell leaves the 10^3 LDS box (cell in [o - 1, o + 7]); and one ulp either side of each."""
    v = np.array(vel, dtype=F)
    N = v.shape[0]
    c = fields.leaves_to_coords(origins).astype(np.float64)
    o = np.repeat(np.asarray(origins, dtype=np.float64), 512, axis=0)
    idx = np.flatnonzero(rng.random(N) < 0.3)
    axis = rng.integers(0, 3, size=len(idx))
    kind = rng.integers(0, 5, size=len(idx))
    side = rng.integers(-1, 2, size=len(idx))
    cc, oo = c[idx, axis], o[idx, axis]
    target = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [cc - rng.integers(-3, 4, size=len(idx)), oo, oo + 8.0, oo - 1.0], oo + 7.0)
    t32 = target.astype(F)
    t32 = np.where(side < 0, np.nextafter(t32, F(-np.inf)), np.where(side > 0, np.nextafter(t32, F(np.inf)), t32))
    v[idx, axis] = ((cc - t32.astype(np.float64)) / SDT).astype(F)
    return v


# ---------------------------------------------------------------------------------------------------------------
# leaf sets
# ---------------------------------------------------------------------------------------------------------------


def ragged32(shift=(0, 0, 0)) -> np.ndarray:
    """32 leaves of a 4 x 4 x 4 lattice around the origin (its leaf included), in NanoVDB order; `shift` in voxels"""
    rng = np.random.default_rng(5)
    lat = np.stack(np.meshgrid(*[np.arange(-2, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    keep = np.argsort(rng.random(len(lat)))[:32]
    keep = np.union1d(keep[:31], [np.flatnonzero((lat == 0).all(1))[0]])  # the origin's leaf is in
    if len(keep) < 32:
        keep = np.union1d(keep, [np.setdiff1d(np.arange(len(lat)), keep)[0]])
    o = (lat[keep] * 8 + np.asarray(shift)).astype(np.int32)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


def sparse_far() -> np.ndarray:
    """sparse_leaves() of tests/test_parity_gpu.py: ~20 leaves straddling the origin and two far tiles at -4104 / +4096"""
    rng = np.random.default_rng(3)
    lat = np.stack(np.meshgrid(*[np.arange(-2, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    o = (lat[rng.random(len(lat)) < 0.3] * 8).astype(np.int32)
    o = np.concatenate([o, np.array([[-4104, 0, 0], [4096, 8, -16]], dtype=np.int32)])
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


def _ordered(o):
    o = np.asarray(o, dtype=np.int32)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


LEAF_SETS = {
    "ragged32": lambda: ragged32(),
    "ragged32_off_origin": lambda: ragged32((96, -104, 80)),  # no leaf within 64 voxels of (0, 0, 0): a NaN position (cell 0) is outside
    "sparse_far": sparse_far,
    "dense32": lambda: _ordered(fields.dense_leaves(32)),  # 16^3 SOR blocks, z-pair divergence
    "one_leaf": lambda: np.array([[8, -16, 24]], dtype=np.int32),
}
# the 7-iteration solve in the `nonfinite` class needs >= 64k voxels for its one planted voxel (NaN share <= half)
LEAF_SETS_BIG = {"dense48": lambda: _ordered(fields.dense_leaves(48))}


# ---------------------------------------------------------------------------------------------------------------
# equalities
# ---------------------------------------------------------------------------------------------------------------


def _words(a):
    return np.ascontiguousarray(np.asarray(a), dtype=F).reshape(-1)


def bit_differences(a, b) -> np.ndarray:
    """positions where a and b differ as 32-bit words, a NaN equal to any NaN"""
    a, b = _words(a), _words(b)
    assert a.shape == b.shape
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))


def same_bits(a, b) -> bool:
    return len(bit_differences(a, b)) == 0


def describe(a, b, limit=6) -> str:
    d = bit_differences(a, b)
    a, b = _words(a), _words(b)
    return f"{len(d)} of {a.size} words differ; first at {d[:limit].tolist()}: {a[d[:limit]].tolist()} vs {b[d[:limit]].tolist()} (hex {[hex(x) for x in a.view(np.uint32)[d[:limit]]]} vs {[hex(x) for x in b.view(np.uint32)[d[:limit]]]})"


def same_but_zero_sign(a, b):
    """(ok, positions): ok if every difference under same_bits is +0 against -0; positions = where those are"""
    d = bit_differences(a, b)
    a, b = _words(a), _words(b)
    z = (a[d] == 0) & (b[d] == 0)
    return bool(z.all()), d[z]


def nan_sign_differences(a, b):
    """For two HIP forms of one kernel: (ok, count). ok: a and b are equal as 32-bit words -- zero signs, subnormals and inf included,
    and a NaN only against a NaN -- except that two NaN may differ in their SIGN BIT; count = how many do. The sign of a NaN result is not
    the source's to choose: a - b is issued as a + (-b) with a negate modifier that flips a NaN operand's sign, and which of two NaN
    operands an add returns depends on the operand order the compiler picked for that form (LLVM leaves both free). Measured on the
    MI355X: the temporally blocked solve against the two-launch form, and stencil = block against the default, differ in exactly such
    words (0x7fc00000 against 0xffc00000) and in nothing else. The payload is asserted equal."""
    a, b = _words(a).view(np.uint32), _words(b).view(np.uint32)
    d = np.flatnonzero(a != b)
    both_nan = ((a[d] & 0x7FFFFFFF) > 0x7F800000) & ((b[d] & 0x7FFFFFFF) > 0x7F800000)
    sign_only = ((a[d] ^ b[d]) == 0x80000000)
    return bool((both_nan & sign_only).all()), int(len(d))


# ---------------------------------------------------------------------------------------------------------------
# one workload = every input of every kernel for (leaf set, class, where)
# ---------------------------------------------------------------------------------------------------------------


class Workload:
    """`speed`: back-trace length in voxels (30: beyond the neighbour tables, the origin-hash path)."""

    def __init__(self, origins, cls, where, seed=0, speed=4.0, rate=0.003):
        assert cls in CLASSES and where in WHERE
        self.origins, self.cls, self.where = np.ascontiguousarray(origins, dtype=np.int32), cls, where
        rng = np.random.default_rng([seed, CLASSES.index(cls), WHERE.index(where)])
        N = self.N = len(self.origins) * 512
        vel = (rng.standard_normal((N, 3)) * (speed / SDT / 2.0)).astype(F)
        phi = [rng.standard_normal(N).astype(F) for _ in range(11)]
        sdf = (rng.standard_normal(N) * 0.5).astype(F)
        sdf[rng.random(N) < 0.2] = F(0.05)  # inside the blend margin
        p0 = rng.standard_normal(N).astype(F)
        div = (rng.standard_normal(N) * 3.0).astype(F)
        temp = (phi[1] * F(30) + F(20)).astype(F)
        fuel, waste, flame = (np.abs(phi[2]) * F(0.3)).astype(F), (np.abs(phi[3]) * F(0.6)).astype(F), np.abs(phi[5])
        in_fields, in_vel = where in ("fields", "both"), where in ("velocity", "both")
        self.planted = {"vel": in_vel, "fields": in_fields}
        if in_vel:
            # (`huge` at 0.4 % of the velocity's values, not 2 %: vorticity confinement reads 37 voxels x 3 components, and at 2 % more than
            # half of the reference's own output is NaN)
            vel = threshold_velocity(vel, self.origins, rng) if cls == "thresholds" else plant(cls, vel, rng, rate, huge_share=0.004)
        if in_fields:
            phi = [plant(cls, p, rng, rate) for p in phi]
            sdf, temp, flame = plant(cls, sdf, rng, rate), plant(cls, temp, rng, rate), plant(cls, flame, rng, rate)
            fuel, waste = plant(cls, fuel, rng, rate), plant(cls, waste, rng, rate)
            if cls == "thresholds":  # oxygen == fuel (1 - f - w == f), oxygen == 0, burn * 10 == 1, each with its neighbours
                k = np.flatnonzero(rng.random(N) < 0.2)
                pairs = [(f_, w_) for f0, w0 in ((0.25, 0.5), (0.5, 0.5), (0.1, 0.0), (0.1, 0.8)) for f_ in _around(f0) for w_ in _around(w0)]
                pick = rng.integers(0, len(pairs), size=len(k))
                fuel[k] = np.array([p[0] for p in pairs], dtype=F)[pick]
                waste[k] = np.array([p[1] for p in pairs], dtype=F)[pick]
            if cls == "nonfinite":
                # the solve spreads a NaN two voxels per iteration: at most four plantings per 16k voxels (one on a single leaf, at
                # its first voxel: a corner, where the cone is an eighth of a ball)
                few = max(1, min(4, N // 4096))
                p0 = plant_few(p0, rng, few) if N > 512 else self._corner(p0)
                div = plant_few(div, rng, few) if N > 512 else div
            else:
                p0, div = plant(cls, p0, rng, rate), plant(cls, div, rng, rate)
        if in_fields or in_vel:
            # element 0 is what advect_scalars reads for every out-of-domain tap (Kernel.cu:133,192,225): give it a special value
            e0 = {"zeros": F(-0.0), "subnormal": SUB_MAX, "huge": F(3e38), "nonfinite": QNAN[0], "thresholds": np.nextafter(F(0), F(1))}[cls]
            if in_fields:
                for p in phi[::2]:
                    p[0] = e0
            if in_vel:
                vel[0, 1] = e0
        self.vel, self.phi, self.sdf, self.p0, self.div, self.temp, self.fuel, self.waste, self.flame = vel, phi, sdf, p0, div, temp, fuel, waste, flame

    @staticmethod
    def _corner(p):
        p = p.copy()
        p[0] = QNAN[0]
        return p


S_LIST = (1, 5, 11)
SOR_ITERS = (1, 2, 3, 4)
KERNEL_OF = {}  # output name -> kernel name


def run_kernels(E, w: Workload, coll: bool, sor_iters=SOR_ITERS) -> dict:
    """Every kernel of the substep on workload `w` through engine `E` (OracleGrid, RefKernelGrid or HipKernels): name -> output.
    The kernels that take no collision field run with coll = False only."""
    out = {}

    def put(kernel, name, a):
        KERNEL_OF[name] = kernel
        out[name] = np.asarray(a)

    s = w.sdf if coll else None
    put("advect_vector", "advect_vector", E.advect_vector(w.vel, DT, INV, s, coll))
    put("advect_scalar", "advect_scalar", E.advect_scalar(w.vel, w.phi[0], DT, INV, s, coll))
    for S in S_LIST:
        for i, a in enumerate(E.advect_scalars(w.vel, w.phi[:S], DT, INV, s, coll)):
            put("advect_scalars", f"advect_scalars S={S} [{i}]", a)
    put("subtract_pressure_gradient", "gradient", E.subtract_pressure_gradient(w.vel, w.p0, INV, s, coll))
    if coll:
        put("enforce_collision_boundaries", "enforce", E.enforce_collision_boundaries(w.vel, w.sdf, float(F(VS))))
        return out
    put("divergence", "divergence", E.divergence(w.vel, INV))
    for K in sor_iters:
        put("rbgs", f"rbgs x{K}", E.rbgs_iterations(w.div, float(F(VS)), OMEGA, K, w.p0))
    for fs in (0.5, 1.0, 2.0):
        put("vorticity_confinement", f"vorticity fs={fs}", E.vorticity_confinement(w.vel, DT, INV, 0.7, fs))
    put("temperature_buoyancy", "buoyancy", E.temperature_buoyancy(w.vel, w.temp, DT, AMBIENT, STRENGTH))
    for n, a in zip(("fuel", "waste", "temperature", "flame", "divergence"), E.combustion_oxygen(w.fuel, w.waste, w.temp, w.div, w.flame, 0.5, 0.1)):
        put("combustion_oxygen", f"combustion {n}", a)
    return out


ADVECTION = ("advect_vector", "advect_scalar", "advect_scalars")
# which planted inputs each kernel reads
READS = {"advect_vector": ("vel",), "advect_scalar": ("vel", "fields"), "advect_scalars": ("vel", "fields"), "subtract_pressure_gradient": ("vel", "fields"),
         "enforce_collision_boundaries": ("vel", "fields"), "divergence": ("vel",), "rbgs": ("fields",), "vorticity_confinement": ("vel",),
         "temperature_buoyancy": ("vel", "fields"), "combustion_oxygen": ("fields",)}


# whose magnitude the output's magnitude follows: a subnormal can only come out where all of these are planted (u - grad p is as
# large as the larger of the two)
CARRIES = {"advect_vector": ("vel",), "advect_scalar": ("fields",), "advect_scalars": ("fields",), "subtract_pressure_gradient": ("vel", "fields"),
           "enforce_collision_boundaries": ("vel",), "divergence": ("vel",), "rbgs": ("fields",), "vorticity_confinement": ("vel",),
           "temperature_buoyancy": ("vel",), "combustion_oxygen": ("fields",)}


def is_subnormal(a):
    a = np.abs(_words(a))
    return (a > 0) & (a < FLT_MIN)


def check_comparator(w: Workload, out: dict):
    """The conditions of a meaningful comparison, asserted on the COMPARATOR's output `out` (never on the kernel under test's):
    at most half of any array is NaN; in `nonfinite` every kernel that reads planted values and does not clamp shows a NaN and a
    finite value; in `subnormal` every kernel whose output follows planted values (CARRIES) puts out at least one subnormal."""
    by_kernel = {}
    for name, a in out.items():
        share = float(np.isnan(a).mean())
        assert share <= 0.5, f"{name}: {share:.2f} of the comparator's values are NaN"
        by_kernel.setdefault(KERNEL_OF[name], []).append(a)
    for kernel, arrays in by_kernel.items():
        if not any(w.planted[r] for r in READS[kernel]):
            continue
        if w.cls == "nonfinite" and kernel not in ADVECTION:
            if kernel == "temperature_buoyancy" and not w.planted["vel"]:
                continue  # fmaxf(0, NaN * strength) = 0 and `t <= ambient` is false for NaN: a NaN temperature is swallowed (Kernel.cu:840-845)
            for name, a in out.items():
                if KERNEL_OF[name] != kernel or name == "combustion flame":  # (flame = fmaxf(flame, fminf(1, burn * 10)) clamps: Kernel.cu:963)
                    continue
                assert np.isnan(a).any() and np.isfinite(a).any(), f"{kernel}: the comparator shows no NaN, or nothing finite"
        if w.cls == "subnormal" and all(w.planted[r] for r in CARRIES[kernel]):
            assert any(is_subnormal(a).any() for a in arrays), f"{kernel}: no subnormal in the comparator's output"


def limiter_swallowed_a_nan(w: Workload, advect_scalar_out) -> int:
    """advect_scalar without collision: the number of output voxels whose first sample's eight corners (around c - SDT * u,
    as the kernel computes it) included a planted NaN and whose output (the comparator's) is finite: the limiter at work."""
    c = fields.leaves_to_coords(w.origins)
    back = (c.astype(F) - F(SDT) * w.vel).astype(F)
    ok = np.isfinite(back).all(1) & (np.abs(back) < 1e6).all(1)
    cell = np.floor(np.where(ok[:, None], back, 0)).astype(np.int64)
    key = lambda ijk: ((ijk[..., 0] >> 3) + (1 << 20)) << 42 | ((ijk[..., 1] >> 3) + (1 << 20)) << 21 | ((ijk[..., 2] >> 3) + (1 << 20))
    leaf_keys = key(w.origins.astype(np.int64))
    order = np.argsort(leaf_keys)
    hit = np.zeros(w.N, dtype=bool)
    phi = w.phi[0]
    for d in range(8):
        t = cell + np.array([d >> 2, (d >> 1) & 1, d & 1])
        k = key(t)
        pos = np.clip(np.searchsorted(leaf_keys[order], k), 0, len(order) - 1)
        leaf = order[pos]
        present = leaf_keys[leaf] == k
        idx = leaf * 512 + (((t[:, 0] & 7) << 6) | ((t[:, 1] & 7) << 3) | (t[:, 2] & 7))
        hit |= present & np.isnan(phi[np.where(present, idx, 0)])
    return int((hit & ok & np.isfinite(_words(advect_scalar_out))).sum())


# ---------------------------------------------------------------------------------------------------------------
# whole operators
# ---------------------------------------------------------------------------------------------------------------
SIM_NAMES = ["density", "temperature", "fuel", "waste", "flame"]


def operator_inputs(origins, cls, seed=0):
    """(vel, fields incl. collision_sdf, projection velocity) for Compute_Sim / ProjectNonDivergent in class `cls`: the smooth
    synthetic state with the class planted into every scalar field and the velocity. `nonfinite` goes where a whole substep
    does not turn it into a flood (the 7-iteration solve spreads every NaN of its right-hand side over a ball of radius 14):
    density and flame for Compute_Sim, at most four velocity components for the projection. `huge` likewise: every scalar field,
    but the velocity only in four components of the projection's (3e37 * 32 overflows in the divergence)."""
    origins = np.ascontiguousarray(origins, dtype=np.int32)
    rng = np.random.default_rng([seed, 77, CLASSES.index(cls)])
    R = 32
    f = fields.synthetic_fields(origins, R)
    N = len(origins) * 512
    cur = {n: f[n].copy() for n in SIM_NAMES}
    vel = f["vel"].copy()
    sdf = np.full(N, 5.0, F)
    sdf[: N // 2] = SDF_FILL  # the state a regrid leaves in new leaves
    sdf[::7] = F(0.05)
    sdf[::13] = F(-0.25)
    few = max(1, min(4, N // 4096))
    if cls == "nonfinite":
        for n in ("density", "flame"):
            cur[n] = plant(cls, cur[n], rng)
        pvel = plant_few(vel, rng, few)
    elif cls == "huge":
        for n in SIM_NAMES:
            cur[n] = plant(cls, cur[n], rng)
        pvel = vel.copy()
        pvel.reshape(-1)[rng.choice(3 * N, size=few, replace=False)] = F(3e37)
    elif cls == "thresholds":
        for n in SIM_NAMES:
            cur[n] = plant(cls, cur[n], rng)
        sdf = plant(cls, sdf, rng)
        vel = threshold_velocity(vel, origins, rng)
        pvel = vel.copy()
    else:
        for n in SIM_NAMES:
            cur[n] = plant(cls, cur[n], rng)
        vel = plant(cls, vel, rng)
        pvel = vel.copy()
    cur["collision_sdf"] = sdf
    return vel, cur, pvel


def run_operators(E, origins, cls, collision, params, iterations=7):
    """name -> array after one Compute_Sim (vorticity on) and one ProjectNonDivergent through engine E"""
    vel, cur, pvel = operator_inputs(origins, cls)
    if not collision:
        del cur["collision_sdf"]
    assert E.compute_sim(vel, cur, iterations, DT, VS, params, collision) == 0
    out = {"vel": vel, **{n: cur[n] for n in SIM_NAMES}}
    assert E.project_non_divergent(pvel, 3, VS) == 0
    out["projected"] = pvel
    return out
