"""The velocity box of k_advect_vector_n, k_advect_vector_n<true> and the look-ahead form of advect_scalars holds its x and y components in
interleaved rows of one plane and z in a second (hns_advect.hip: kVCy, kVCz). A row, a component or a shell cell that lands in the wrong place
changes a tap of the second sample or a clamp neighbour; every comparison here is equality of 32-bit words, nothing is a tolerance.

Grids, the smallest at which the layout can go wrong: one leaf alone (every shell cell outside the domain, where advect_vector's box holds 0 and
the fields' boxes element g.oob); 3 x 3 x 3 leaves without one face, one edge and one corner neighbour of the centre; 4 x 4 x 4 dense. Each
velocity component has its own offset and scale, so that a swapped or shifted component cannot cancel. Below one voxel per step both second
samples are read from the boxes; above eight the taps leave the box and the 27-leaf neighbourhood (gather and far paths). S = 1 and 2: both
field boxes alternate. Two core substeps: the second consumes what the first looked ahead.

Per case one run of the 64-bit kernels (advect = generic), which hold no box, is the reference; advect = auto with lookahead = 0
(k_advect_vector_n) and with lookahead = 1 (k_advect_scalars_n<false, true>) are compared with it, and so with each other."""
import functools

import numpy as np
import pytest

from frame_cases import download, make_sim
from hnanosolver_amd import fields

pytestmark = pytest.mark.gpu

DT = float(np.float32(1.0 / 24.0))
VS = 1.0 / 32
ITERS = 2
NAMES = ["density", "temperature"]


def lattice(n, without=()):
    l = np.arange(n, dtype=np.int32)
    o = np.stack(np.meshgrid(l, l, l, indexing="ij"), axis=-1).reshape(-1, 3)
    keep = np.array([tuple(x) not in set(without) for x in o.tolist()])
    o = np.ascontiguousarray(o[keep] * 8, dtype=np.int32)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)], dtype=np.int32)


GRIDS = {
    "one_leaf": lambda: lattice(1),
    # centre (1, 1, 1): face neighbour +x, edge neighbour -y -z, corner neighbour -x +y +z removed
    "holes27": lambda: lattice(3, without=[(2, 1, 1), (1, 0, 0), (0, 2, 2)]),
    "dense64": lambda: lattice(4),
}
AMPLITUDES = {"slow": 0.6, "fast": 11.0}  # voxels per step, the largest component


def start_state(origins, voxels_per_step):
    """velocity in world units per second: |component| * DT / VS voxels per step; x, y and z differ in offset, scale and wave number"""
    c = fields.leaves_to_coords(origins).astype(np.float64)
    rng = np.random.default_rng(5)
    a = voxels_per_step * VS / DT
    vel = np.stack(
        [
            a * (0.55 + 0.45 * np.sin(0.9 * c[:, 1] + 0.3 * c[:, 2])),
            a * (-0.35 + 0.3 * np.cos(0.7 * c[:, 0] - 0.4 * c[:, 2])),
            a * (0.15 - 0.6 * np.sin(0.5 * c[:, 0] + 0.8 * c[:, 1])),
        ],
        axis=1,
    )
    vel = (vel + 0.03 * a * rng.standard_normal(vel.shape)).astype(np.float32)
    st = {"vel": vel}
    for i, n in enumerate(NAMES):
        st[n] = (np.cos(0.6 * c[:, 0] + 0.2 * i) * np.sin(0.5 * c[:, 1] + 0.7 * c[:, 2]) + 0.1 * rng.standard_normal(len(c)) + 3.0 * i).astype(np.float32)
        st[n][0] = 50.0 + i  # element g.oob = 0: what the fields' taps and shell cells read outside the domain
    return st


@functools.lru_cache(maxsize=None)
def run(grid, amplitude, S, advect, lookahead):
    import hnanosolver_amd as H

    names = NAMES[:S]
    o = GRIDS[grid]()
    st = start_state(o, AMPLITUDES[amplitude])
    H.set_option("advect", advect)
    H.set_option("lookahead", lookahead)
    try:
        g, s = make_sim(o, names, {k: st[k] for k in ["vel"] + names}, None, VS)
        snaps = []
        for _ in range(2):
            s.core_substep(ITERS, DT, VS)
            snaps.append(download(s, names))
        counts = s.lookahead_counts()
        s.close()
    finally:
        H.set_option("advect", None)
        H.set_option("lookahead", None)
    return snaps, counts


def assert_words(got, want, what):
    g, w = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32) for a in (got, want))
    d = np.flatnonzero(g != w)
    print(f"{what}: {len(d)} of {g.size} words differ")
    assert len(d) == 0, f"{what}: {len(d)} of {g.size} words differ; first at {d[:6].tolist()}: {[hex(x) for x in g[d[:6]]]} vs {[hex(x) for x in w[d[:6]]]}"


def assert_same_runs(got, want, what):
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.keys() == y.keys()
        for k in x:
            assert_words(x[k], y[k], f"{what}: substep {i} {k}")


CASES = [(g, a, S) for g in GRIDS for a in AMPLITUDES for S in (1, 2)]


@pytest.mark.parametrize("grid,amplitude,S", CASES)
def test_boxed_vector_kernel_equals_generic(grid, amplitude, S):
    """advect = auto (k_advect_vector_n: both samples and the clamp out of the box) against advect = generic"""
    want, _ = run(grid, amplitude, S, "generic", "0")
    got, counts = run(grid, amplitude, S, "auto", "0")
    assert counts == (0, 0)
    assert_same_runs(got, want, f"{grid} {amplitude} S={S} auto vs generic")


@pytest.mark.parametrize("grid,amplitude,S", CASES)
def test_lookahead_equals_two_launches(grid, amplitude, S):
    """lookahead = 1 (the velocity box of the look-ahead form, consumed by the second substep) against lookahead = 0"""
    want, _ = run(grid, amplitude, S, "auto", "0")
    got, counts = run(grid, amplitude, S, "auto", "1")
    assert counts == (2, 1)  # both substeps looked ahead, the second found its advect_vector done
    assert_same_runs(got, want, f"{grid} {amplitude} S={S} lookahead 1 vs 0")


def test_the_states_exercise_what_they_claim():
    """the slow state stays below one voxel per step in every component, the fast one passes eight; the components differ"""
    o = GRIDS["dense64"]()
    for name, lo, hi in (("slow", 0.0, 1.0), ("fast", 8.0, 1e9)):
        v = np.abs(start_state(o, AMPLITUDES[name])["vel"].astype(np.float64)) * DT / VS
        print(name, v.max(axis=0))
        assert lo < v.max() < hi
    m = start_state(o, 1.0)["vel"].mean(axis=0)
    assert abs(m[0] - m[1]) > 0.3 * VS / DT and abs(m[1] - m[2]) > 0.3 * VS / DT
