"""TEST HELPER of tests/test_shaping_cases.py (CPU) and tests/test_shaping_gpu.py: the mirror of hns_shaping_apply and hns_shaping_curl_host restated from the text of
include/hns.h ("SHAPING A SIM") alone, not from hns_noise.hpp: numpy float32, one rounded operation per line, uint32 integers that wrap. `cell_curl` is written once over
a dtype, so the float64 restatement the mathematics is held in (noise values, analytic gradient, curl; tests/test_shaping_cases.py) is the same text at another
precision; `potential` (N itself, which the kernel never forms) exists for that test's central differences only."""
import numpy as np

F = np.float32
U = np.uint32
FAR = F(4194304.0)

# the 16 gradients of improved Perlin noise, in the header's order
TABLE = np.array([(1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1),
                  (1, 1, 0), (-1, 1, 0), (0, -1, 1), (0, -1, -1)], dtype=np.float64) + 0.0  # (+ 0.0: every zero is +0)

SPEC = dict(amplitude=0.0, frequency=1.0 / 16, offset=(0.0, 0.0, 0.0), octaves=1, lacunarity=2.0, gain=0.5, seed=0, control=None, control_lo=0.0, control_hi=1.0)


def spec_of(**over):
    unknown = set(over) - set(SPEC)
    assert not unknown, unknown
    return {**SPEC, **over}


def H(x):
    """birth_hash (include/hns.h: BIRTH AND DEATH OF POINTS)"""
    x = np.asarray(x, dtype=U).copy()
    x ^= x >> U(16)
    x *= U(0x7FEB352D)
    x ^= x >> U(15)
    x *= U(0x846CA68B)
    x ^= x >> U(16)
    return x


def octave_constants(spec):
    """[(f_o, a_o, s_o)] in float32 / uint32"""
    out = []
    f, a = F(spec["frequency"]), F(1.0)
    with np.errstate(over="ignore"):
        base = H(U(spec["seed"] & 0xFFFFFFFF) ^ U(0x9E3779B9))
        for o in range(spec["octaves"]):
            if o:
                f, a = F(f * F(spec["lacunarity"])), F(a * F(spec["gain"]))
            out.append((f, a, H(base + U(o))))
    return out


def lerp(v0, v1, w):
    d = v1 - v0
    d = w * d
    return v0 + d


def fade(t, T):
    a = T(6.0) * t
    a = a - T(15.0)
    a = a * t
    a = a + T(10.0)
    a = a * t
    a = a * t
    return a * t


def fade_slope(t, T):
    b = t - T(2.0)
    b = b * t
    b = b + T(1.0)
    e = T(30.0) * t
    e = e * t
    return e * b


def corner_values(I, t, s, T):
    """g [3 channels][2, 2, 2, n, 3] and d [3][2, 2, 2, n] of the eight corners of cells I ([n, 3] int32) with fractions t ([n, 3] of dtype T)"""
    n = len(I)
    g = np.empty((3, 2, 2, 2, n, 3), T)
    d = np.empty((3, 2, 2, 2, n), T)
    table = TABLE.astype(T)
    with np.errstate(over="ignore"):
        for a in (0, 1):
            for b in (0, 1):
                for e in (0, 1):
                    h = H(H(H(s ^ (I[:, 0] + a).astype(np.int32).astype(U)) ^ (I[:, 1] + b).astype(np.int32).astype(U)) ^ (I[:, 2] + e).astype(np.int32).astype(U))
                    p = [t[:, 0] if a == 0 else t[:, 0] - T(1.0), t[:, 1] if b == 0 else t[:, 1] - T(1.0), t[:, 2] if e == 0 else t[:, 2] - T(1.0)]
                    for m in range(3):
                        gm = table[(h >> U(4 * m)) & U(15)]
                        g[m, a, b, e] = gm
                        dx, dy, dz = gm[:, 0] * p[0], gm[:, 1] * p[1], gm[:, 2] * p[2]
                        d[m, a, b, e] = (dx + dy) + dz
    return g, d


def nest8(v, u):
    """L(v): z, then y, then x"""
    vz = lerp(v[:, :, 0], v[:, :, 1], u[2])
    vy = lerp(vz[:, 0], vz[:, 1], u[1])
    return lerp(vy[0], vy[1], u[0])


def partial(d, g, u, du, axis):
    """dN/d(axis) of one channel: d [2, 2, 2, n], g [2, 2, 2, n, 3]"""
    if axis == 0:
        D = d[1] - d[0]                    # [b, e]
        D = lerp(D[:, 0], D[:, 1], u[2])   # z
        D = lerp(D[0], D[1], u[1])         # y
    elif axis == 1:
        D = d[:, 1] - d[:, 0]              # [a, e]
        D = lerp(D[:, 0], D[:, 1], u[2])   # z
        D = lerp(D[0], D[1], u[0])         # x
    else:
        D = d[:, :, 1] - d[:, :, 0]        # [a, b]
        D = lerp(D[:, 0], D[:, 1], u[1])   # y
        D = lerp(D[0], D[1], u[0])         # x
    L = nest8(g[..., axis], u)
    m = du[axis] * D
    return m + L


def cell_curl(I, t, s, T=F, gradient=False):
    """c_o of cells I with fractions t for the octave seed s, [n, 3] of dtype T. gradient: instead all nine partials [n, 3 channels, 3 axes] (the float64 test)"""
    t = np.asarray(t, dtype=T)
    g, d = corner_values(np.asarray(I), t, s, T)
    u = [fade(t[:, c], T) for c in range(3)]
    du = [fade_slope(t[:, c], T) for c in range(3)]
    P = lambda m, axis: partial(d[m], g[m], u, du, axis)
    if gradient:
        return np.stack([np.stack([P(m, axis) for axis in range(3)], -1) for m in range(3)], 1)
    return np.stack([P(2, 1) - P(1, 2), P(0, 2) - P(2, 0), P(1, 0) - P(0, 1)], -1)


def potential(I, t, s, T=np.float64):
    """(N_0, N_1, N_2) [n, 3]: L(d_abe), for the central differences of the float64 test only"""
    t = np.asarray(t, dtype=T)
    g, d = corner_values(np.asarray(I), t, s, T)
    u = [fade(t[:, c], T) for c in range(3)]
    return np.stack([nest8(d[m], u) for m in range(3)], -1)


def lattice(f, offset, ijk):
    """near [n] (no component under the far rule), I [n, 3] int32 and t [n, 3] float32 of octave frequency f"""
    with np.errstate(over="ignore", invalid="ignore"):
        q = F(f) * np.asarray(ijk, dtype=np.int32).astype(F)
        q = q + np.asarray(offset, dtype=F)[None, :]
        near = (np.abs(q) < FAR).all(1)  # (a NaN and an infinity compare false)
    qn = np.where(near[:, None], q, F(0.0))
    I = np.floor(qn).astype(np.int32)
    t = qn - I.astype(F)
    return near, I, t


def curl(spec, ijk):
    """C of the voxels ijk [n, 3] (global coordinates): what hns_shaping_curl_host returns, [n, 3] float32"""
    ijk = np.asarray(ijk, dtype=np.int32).reshape(-1, 3)
    C = np.zeros((len(ijk), 3), F)
    for f, a, s in octave_constants(spec):
        near, I, t = lattice(f, spec["offset"], ijk)
        c = np.zeros((len(ijk), 3), F)
        if near.any():
            c[near] = cell_curl(I[near], t[near], s)
        e = a * c
        C = C + e
    return C


def apply_mirror(ijk, vel, fields, dt, turbulence=None, decay=None):
    """hns_shaping_apply on the voxels ijk [n, 3]: (vel', fields') as new arrays; fields: {name: [n] float32}; decay: {name: (rate, target)}"""
    vel, fields = np.array(vel, dtype=F), {k: np.array(v, dtype=F) for k, v in fields.items()}
    dt = F(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        if turbulence is not None and F(turbulence["amplitude"]) != 0:
            C = curl(turbulence, ijk)
            kA = F(turbulence["amplitude"]) * dt
            if turbulence["control"] is None:
                k = np.full(len(vel), kA, F)
            else:
                inv = F(1.0) / (F(turbulence["control_hi"]) - F(turbulence["control_lo"]))
                w = fields[turbulence["control"]] - F(turbulence["control_lo"])
                w = w * inv
                w = np.where(w > 0, w, F(0.0))  # the GPU's max: a NaN loses; -0 gives +0
                w = np.where(w < 1, w, F(1.0))
                k = kA * w
            e = k[:, None] * C
            vel = vel + e
        for name, (rate, target) in (decay or {}).items():
            r = F(1.0) / (F(1.0) + F(rate) * dt)
            t = fields[name] - F(target)
            t = t * r
            fields[name] = F(target) + t
    return vel, fields
