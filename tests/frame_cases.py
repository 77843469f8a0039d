"""The frame loop's test cases, shared by the regrid, source, deactivation and pool-content tests: mask packing, random leaf sets, masks, fields and sources,
device sims, the host chain every device regrid must match byte for byte, and a device-resident sim's frame loop against that chain continued on the host."""
import contextlib

import numpy as np

from hnanosolver_amd import api, device, leafio

COMBUST = ["density", "fuel", "waste", "temperature", "flame"]


def pack(bits: np.ndarray) -> np.ndarray:
    """(n, 512) bool in x<<6|y<<3|z order -> (n, 64) bytes: byte x*8+y, bit z"""
    return np.packbits(bits.reshape(len(bits), 64, 8), axis=2, bitorder="little").reshape(len(bits), 64)


def unpack(masks: np.ndarray) -> np.ndarray:
    return np.unpackbits(masks.reshape(len(masks), 64, 1), axis=2, bitorder="little").reshape(len(masks), 512).astype(bool)


def random_leaves(seed, n=30, span=4):
    rng = np.random.default_rng(seed)
    o = np.unique(rng.integers(-span, span, size=(n, 3)), axis=0).astype(np.int32) * 8
    o = np.concatenate([o, np.array([[8 * 3 * span, -8 * 2 * span, 8]], dtype=np.int32)])  # a lone leaf
    return o[rng.permutation(len(o))]  # caller order, not OpenVDB order


def random_masks(seed, n):
    rng = np.random.default_rng(seed)
    bits = rng.random((n, 512)) < rng.choice([0.003, 0.05, 0.5, 1.0], size=(n, 1))
    bits[: max(1, n // 8)] = False  # leaves without active voxels
    bits[-1, 200] = True
    return pack(bits)


def with_negative_zeros(rng, v):
    v[rng.random(v.shape) < 0.05] = -0.0  # a sum turns these into +0.0 where the other side lacks the leaf; a copy keeps them
    return v


def random_state(seed, n_leaves, names):
    rng = np.random.default_rng(seed)
    st = {"vel": with_negative_zeros(rng, rng.standard_normal((n_leaves * 512, 3)).astype(np.float32))}
    for n in names:
        st[n] = with_negative_zeros(rng, rng.standard_normal(n_leaves * 512).astype(np.float32))
    return st


def make_sim(origins, names, state, masks=None, vs=1.0 / 32):
    g = api.create_grid_from_leaves(origins, vs)
    s = device.Sim(g, names)
    s.upload(state)
    if masks is not None:
        s.set_active_masks(masks)
    return g, s


def download(sim, names):
    n = sim.grid.voxel_count()
    out = {"vel": np.empty((n, 3), dtype=np.float32)}
    for k in names:
        out[k] = np.empty(n, dtype=np.float32)
    sim.download(out)
    return out


def assert_same(a, b, what=""):
    for k in a:
        assert a[k].view(np.uint32).tobytes() == b[k].view(np.uint32).tobytes(), f"{what}: field {k} differs"


def sdf_source(seed, origins, n=6):
    rng = np.random.default_rng(seed)
    so = np.unique(np.concatenate([origins[:2], rng.integers(-8, 8, size=(n, 3)).astype(np.int32) * 8]), axis=0).astype(np.int32)
    so = so[rng.permutation(len(so))]
    sm = pack(rng.random((len(so), 512)) < 0.1)
    sv = rng.standard_normal(len(so) * 512).astype(np.float32)
    return so, sm, sv


def is_velocity(values):
    return values.ndim == 2 and values.shape[1] == 3


def host_chain(origins, masks, state, names, p, sources=None, sdf=None):
    """What a host caller does between two frames, from leafio's functions (hns_add_leaves per source -> hns_dilate_leaf_masks of the summed
    velocity -> union with the SDF's leaves -> hns_gather_leaves): -> (origins, masks, state)"""
    vel_o, vel_m, vel_v = origins, masks, state["vel"]
    cur = {n: (origins, state[n]) for n in names}
    for name, (so, sm, sv) in (sources or {}).items():
        if is_velocity(sv):
            vel_o, vel_m, vel_v = leafio.add_leaves((origins, masks, state["vel"]), (so, sm, sv), 3)
        else:
            o2, _, v2 = leafio.add_leaves((origins, None, state[name]), (so, sm, sv), 1)
            cur[name] = (o2, v2)
    dom, dm = leafio.dilate_leaf_masks(vel_o, p, vel_m)
    if sdf is not None:
        so, sm, sv = sdf
        dom2 = leafio.union_leaves(dom, so)
        m2 = np.zeros((len(dom2), 64), dtype=np.uint8)
        idx = {tuple(o): i for i, o in enumerate(dom2.tolist())}
        for o, m in zip(dom.tolist(), dm):
            m2[idx[tuple(o)]] |= m
        for i, o in enumerate(np.asarray(so).tolist()):
            m2[idx[tuple(o)]] |= 0xFF if sm is None else sm[i]
        dom, dm = dom2, m2
    out = {"vel": leafio.gather_leaves(dom, vel_o, vel_v, 3, leafio.FILL_ZERO)}
    for n in names:
        if n == "collision_sdf" and sdf is not None:
            out[n] = leafio.gather_leaves(dom, sdf[0], sdf[2], 1, leafio.FILL_SDF)
        else:
            out[n] = leafio.gather_leaves(dom, cur[n][0], cur[n][1], 1, leafio.FILL_SDF if n == "collision_sdf" else leafio.FILL_ZERO)
    return dom, dm, out


def host_deactivate(masks, st, tolerances, velocity):
    return leafio.deactivate_masks(masks, {k: (st[k], t) for k, t in tolerances.items()}, None if velocity is None else (st["vel"], velocity))


def frame_chain(s, names, start, frames, inputs, step, tolerances, vtol, vs, shadows=(), keep=None, probe=None):
    """`frames` frames of the device-resident sim `s` -- a sourced regrid, two substeps, a deactivation -- each against the host chain continued on the host with the
    downloaded substep results of a fresh sim: origins and masks after the regrid, deactivation counts, masks and every field after the frame.
    start = (origins, masks or None, state) as uploaded to `s`; inputs(frame, origins) -> (padding, sdf or None, sources); step(sim, frame) runs one substep;
    `shadows` are sims taken through the same regrids and substeps without deactivation; the grids go to `keep` (a list), so that none is freed mid-chain.
    -> per frame (origins, masks after the regrid, masks after the deactivation, its counts, the downloaded fields, probe(s) taken behind the substeps)"""
    ho, hm, hst = start
    keep = [] if keep is None else keep
    out = []
    for frame in range(frames):
        p, sdf, src = inputs(frame, ho)
        keep.append(s.regrid(p, sdf, src))
        for t in shadows:
            keep.append(t.regrid(p, sdf, src))
        ho, hm, hst = host_chain(ho, hm, hst, names, p, src, sdf)
        assert np.array_equal(s.grid.coords()[::512], ho) and np.array_equal(s.active_masks(), hm), f"frame {frame} regrid"
        hg, hs = make_sim(ho, names, hst, None, vs)
        for _ in range(2):
            for sim in (s, *shadows, hs):
                step(sim, frame)
        hst = download(hs, names)
        hs.close()
        probed, regrid_masks = probe(s) if probe else None, hm
        counts = s.deactivate(tolerances, vtol, counts=True)
        hm, hc = host_deactivate(hm, hst, tolerances, vtol)
        assert counts == hc and np.array_equal(s.active_masks(), hm), f"frame {frame} deactivate"
        got = download(s, names)
        assert_same(got, hst, f"frame {frame}")
        out.append((ho, regrid_masks, hm, counts, got, probed))
    return out


def source_leaves(rng, origins, where, n=10):
    """n leaves inside the sim's domain, outside it, or straddling its edge (half of each)"""
    inside = origins[rng.choice(len(origins), size=min(n, len(origins)), replace=False)]
    lat = np.stack(np.meshgrid(np.arange(4, 8), np.arange(-2, 2), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3) * 8  # x in [32, 64): beyond span 4
    outside = lat[rng.choice(len(lat), size=n, replace=False)].astype(np.int32)
    if where == "inside":
        o = inside
    elif where == "outside":
        o = outside
    else:
        o = np.concatenate([inside[: n // 2], outside[: n - n // 2]])
    return np.unique(o, axis=0).astype(np.int32)[rng.permutation(len(np.unique(o, axis=0)))]


def make_sources(seed, origins, kind, where):
    rng = np.random.default_rng(seed)
    out = {}
    if kind in ("velocity", "mixed"):
        o = source_leaves(rng, origins, where)
        m = None if seed % 2 else random_masks(seed + 5, len(o))
        out["vel"] = (o, m, with_negative_zeros(rng, rng.standard_normal((len(o) * 512, 3)).astype(np.float32)))
    if kind in ("float", "mixed"):
        for name in ("density", "temperature"):
            o = source_leaves(rng, origins, where, 7)
            m = random_masks(seed + 7, len(o)) if name == "density" else None  # (masks of a float source do not enter the domain)
            out[name] = (o, m, with_negative_zeros(rng, rng.standard_normal(len(o) * 512).astype(np.float32)))
    return out


LAUNCH_RANGES = ("inner", "half")


@contextlib.contextmanager
def launch_range(grid, kind):
    """the grid's launch range narrowed for the block, the whole range back afterwards (also after a failure) -- "inner": set_active_range on a strict inner range,
    leaves left out at either end; "half": set_active_leaves(n // 2). The point calls count every leaf whatever the range (include/hns.h): ghost leaves included."""
    n = grid.leaf_count()
    edge = max(1, n // 5)
    assert n >= 4 and 0 < edge and edge + (n - 2 * edge) < n
    if kind == "inner":
        grid.set_active_range(edge, n - 2 * edge)
    else:
        assert kind == "half"
        grid.set_active_leaves(n // 2)
    assert grid.active_leaves() == (n - 2 * edge if kind == "inner" else n // 2)
    try:
        yield
    finally:
        grid.set_active_range(0, n)


def emitter(R, frame):
    """velocity, density, temperature and fuel over a box of 2^3 leaves, half of it beyond the +x face of the R^3 domain"""
    lat = np.stack(np.meshgrid(np.arange(-1, 1), np.arange(0, 2), np.arange(0, 2), indexing="ij"), -1).reshape(-1, 3)
    o = ((lat + np.array([R // 8, R // 16 - 1, R // 16 - 1])) * 8).astype(np.int32)
    rng = np.random.default_rng(100 + frame)
    bits = np.zeros((len(o), 512), dtype=bool)
    bits[:, :256] = True  # x < 4 of every leaf
    src = {"vel": (o, pack(bits), (rng.random((len(o) * 512, 3)) * np.float32(0.5)).astype(np.float32))}
    for name in ("density", "temperature", "fuel"):
        src[name] = (o, None, rng.random(len(o) * 512).astype(np.float32))
    return src
