"""Shaping a device-resident sim on the GPU: hns_shaping_apply (k_shape of hns_shaping.hip) through device.Shaping and Sim.shape, against the numpy mirror of
tests/shaping_cases.py, which restates include/hns.h. There is no tolerance anywhere: the velocity and every float field are compared as 32-bit words, on a random sparse
grid of some twenty leaves with negative origins plus two leaves far out, where the far rule cuts through a leaf; the fields hold ordinary values and NaN, +-inf and
zeros of both signs. What the host evaluation of the same header computes is held without a GPU by tests/test_shaping_cases.py.

Not here: the refusal of a lent sim (one that belongs to a grid's cook cache). `cached` and `in_use` are set only inside the cook cache of hns_api.hip and no call of the ABI
hands such a sim out, so no test can reach that refusal; it is the check_sim that the point calls share. And the frequencies still span lattice cells from 16 voxels
to less than one, but they no longer select kernel paths: the LDS-box form they were chosen for lost its measurement and is gone."""
import functools
import time

import numpy as np
import pytest

import shaping_cases as sc
from diag_cases import read_field
from frame_cases import download, make_sim, random_leaves
from hnanosolver_amd import _lib, device

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 32
DT = 0.04
NAMES = ["density", "temperature", "fuel", "waste", "flame", "soot", "heat", "dust", "collision_sdf"]
DECAYABLE = NAMES[:8]
# (2^25 - 8, ..): at frequency 0.125 voxel 0 has q = 2^22 - 1 and voxel 7 rounds to 2^22 -- the far rule cuts through the leaf; (2^26 - 8, ..): the same at 1 / 16
FAR_LEAVES = np.array([[2 ** 25 - 8, 8, -8], [2 ** 26 - 8, 0, 0]], np.int32)


@functools.lru_cache(maxsize=None)
def origins():
    o = np.concatenate([random_leaves(7, n=20, span=3), FAR_LEAVES]).astype(np.int32)
    assert 18 <= len(o) <= 24 and (o < 0).any()
    return o


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_words(got, want, what):
    g, w = words(got).reshape(len(got), -1), words(want).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(1))
    assert not len(bad), f"{what}: {len(bad)} of {len(g)} voxels differ, first {bad[:4].tolist()}: {np.asarray(got)[bad[:4]].tolist()} vs {np.asarray(want)[bad[:4]].tolist()}"


@functools.lru_cache(maxsize=None)
def start_state():
    """ordinary values with NaN, +-inf and zeros of both signs planted in the velocity and in every field; "density" runs from below 0 to above 1 for the control"""
    n = len(origins()) * 512
    rng = np.random.default_rng(11)
    st = {"vel": rng.standard_normal((n, 3)).astype(F)}
    for i, k in enumerate(NAMES):
        st[k] = (rng.standard_normal(n) * (i + 1)).astype(F)
    st["density"] = rng.uniform(-0.5, 1.5, n).astype(F)
    for a in st.values():
        flat = a.reshape(-1)
        for value in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            flat[rng.random(flat.size) < 0.01] = value
    for a in st.values():
        a.setflags(write=False)
    return st


def fresh_sim(state=None, near_only=False):
    """(grid, sim) holding `state` (None: start_state). near_only: without the two far leaves, which are the last two -- the state's rows are cut to match"""
    o = origins()[:-2] if near_only else origins()
    return make_sim(o, NAMES, {k: np.array(v[:len(o) * 512]) for k, v in (state or start_state()).items()}, None, VS)


def everything(sim):
    """the velocity, every field, the divergence and the pressure buffer, as the device holds them"""
    import torch

    torch.cuda.synchronize()
    out = download(sim, NAMES)
    n = sim.grid.leaf_count()
    out["div"] = read_field(_lib.lib.hns_sim_divergence_ptr(sim._ptr), n)
    out["p"] = read_field(_lib.lib.hns_sim_pressure_ptr(sim._ptr), n)
    return out


def expected(before, ijk, dt, turbulence, decay, rows=None):
    """the mirror on `before` (rows: the voxels a narrowed launch range updates; None = all)"""
    vel, fields = sc.apply_mirror(ijk, before["vel"], {k: before[k] for k in NAMES}, dt, turbulence, decay)
    want = {k: np.array(v) for k, v in before.items()}
    rows = slice(None) if rows is None else rows
    want["vel"][rows] = vel[rows]
    for k in NAMES:
        want[k][rows] = fields[k][rows]
    return want


def check(sim, before, turbulence, decay, what, rows=None, dt=DT):
    ijk = sim.grid.coords()
    sim.shape(dt, turbulence, decay)
    got, want = everything(sim), expected(before, ijk, dt, turbulence, decay, rows)
    for k in want:
        assert_words(got[k], want[k], f"{what}: {k}")
    return got


TURBULENCE = {
    "wide": sc.spec_of(amplitude=3.0, frequency=1.0 / 16, octaves=4, lacunarity=2.0, gain=0.5, seed=5, offset=(0.0, 0.5, -17.125)),
    "wide, t = 0": sc.spec_of(amplitude=-2.0, frequency=0.125, octaves=1, seed=6),
    "fine": sc.spec_of(amplitude=3.0, frequency=1.7, octaves=2, lacunarity=2.0, gain=0.75, seed=7, offset=(0.25, -0.5, 2.0)),
    "mixed": sc.spec_of(amplitude=1.5, frequency=0.9, octaves=3, lacunarity=2.0, gain=0.5, seed=8, offset=(-0.125, 0.0, 0.375)),
    "near 8/7": sc.spec_of(amplitude=1.0, frequency=1.14, octaves=2, lacunarity=1.01, gain=1.0, seed=9),
}


@pytest.fixture(scope="module")
def sim():
    g, s = fresh_sim()
    yield s
    s.close()


@pytest.mark.parametrize("case", sorted(TURBULENCE))
def test_turbulence_alone_equals_the_mirror(sim, case):
    """lattice cells of 16 voxels down to less than one, one to four octaves, t = 0 on every leaf corner, offsets of both signs"""
    spec = TURBULENCE[case]
    sim.upload({k: np.array(v) for k, v in start_state().items()})
    before = everything(sim)
    got = check(sim, before, spec, None, case)
    changed = (words(got["vel"]) != words(before["vel"])).any(1)
    assert changed.mean() > 0.8  # (NaN, inf and the far voxels keep their words)
    near = np.stack([sc.lattice(f, spec["offset"], sim.grid.coords())[0] for f, _, _ in sc.octave_constants(spec)])
    assert (~near).any() and near.all(0).sum() >= (len(origins()) - 2) * 512, "the far rule is not met, or met beyond the two far leaves"
    if case.startswith("wide"):
        cut = (~near[0]).reshape(-1, 512)
        assert ((cut.any(1)) & (~cut.all(1))).any(), "no leaf is cut by the far rule"


def test_a_control_field_weights_the_turbulence(sim):
    """the control's voxels fall below lo, inside the range, above hi, and hold NaN, inf and zeros; a control that is collision_sdf is allowed"""
    st = start_state()
    c = st["density"]
    lo, hi = 0.25, 0.75
    assert (c < lo).any() and ((c > lo) & (c < hi)).any() and (c > hi).any() and np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c == 0).any()
    for name, (a, b) in (("density", (lo, hi)), ("collision_sdf", (-1.0, 2.0)), ("density", (0.0, 1e-30))):
        sim.upload({k: np.array(v) for k, v in st.items()})
        before = everything(sim)
        spec = {**TURBULENCE["mixed"], "control": name, "control_lo": a, "control_hi": b}
        got = check(sim, before, spec, None, f"control {name} [{a}, {b}]")
        kept = (words(got["vel"]) == words(before["vel"])).all(1)
        nan_c = np.isnan(before[name])
        assert kept[nan_c & np.isfinite(before["vel"]).all(1)].mean() > 0.3  # a NaN control: w = 0, v + (+0) keeps every finite v but -0


@pytest.mark.parametrize("count", [1, 8])
def test_decay_alone_equals_the_mirror(sim, count):
    sim.upload({k: np.array(v) for k, v in start_state().items()})
    before = everything(sim)
    decay = {k: (0.5 + i, float(i) - 2.5) for i, k in enumerate(DECAYABLE[:count])}
    if count == 8:
        decay["fuel"] = (0.0, 1.0)  # rate 0: r = 1
    got = check(sim, before, None, decay, f"{count} decays")
    assert (words(got[DECAYABLE[count - 1]]) != words(before[DECAYABLE[count - 1]])).mean() > 0.9


def test_both_together_and_the_weight_comes_from_the_control_before_its_decay(sim):
    sim.upload({k: np.array(v) for k, v in start_state().items()})
    before = everything(sim)
    spec = {**TURBULENCE["mixed"], "control": "density", "control_lo": 0.25, "control_hi": 0.75}
    decay = {"temperature": (2.0, 0.5), "density": (30.0, -4.0)}
    check(sim, before, spec, decay, "turbulence and decay")
    # the mirror with the weight taken AFTER the decay is another velocity: the comparison above tells the two apart
    _, decayed = sc.apply_mirror(sim.grid.coords(), before["vel"], {k: before[k] for k in NAMES}, DT, None, decay)
    late, _ = sc.apply_mirror(sim.grid.coords(), before["vel"], {**{k: before[k] for k in NAMES}, "density": decayed["density"]}, DT, spec, None)
    early, _ = sc.apply_mirror(sim.grid.coords(), before["vel"], {k: before[k] for k in NAMES}, DT, spec, None)
    assert (words(late) != words(early)).any(1).mean() > 0.3


def test_no_amplitude_leaves_the_velocity_and_the_memo_and_nothing_at_all_launches_nothing():
    """amplitude = 0 with decays: the velocity's bytes stay and the next substep still consumes the look-ahead memo; with nothing to do the call returns at once"""
    import hnanosolver_amd as H

    clean = {k: np.nan_to_num(np.array(v), nan=0.5, posinf=1.0, neginf=-1.0) for k, v in start_state().items()}
    H.set_option("lookahead", "1")
    try:
        g1, a = fresh_sim(clean, near_only=True)
        a.core_substep(3, DT, VS)
        assert a.lookahead_counts()[0] >= 1
        before = everything(a)
        got = check(a, before, {**TURBULENCE["wide"], "amplitude": 0.0}, {"density": (1.0, 0.0)}, "amplitude 0")
        assert_words(got["vel"], before["vel"], "amplitude 0: vel")
        a.shape(DT, None, None), a.shape(DT, {**TURBULENCE["wide"], "amplitude": -0.0}, {})
        for k, v in everything(a).items():
            assert_words(v, got[k], f"a call with nothing to do: {k}")
        g2, twin = fresh_sim({k: got[k] for k in ["vel"] + NAMES}, near_only=True)
        for s in (a, twin):
            s.core_substep(3, DT, VS)
        assert a.lookahead_counts()[1] >= 1, "the memo was dropped by a call that wrote no velocity"
        after, after_twin = download(a, NAMES), download(twin, NAMES)
        for k in after:
            assert_words(after[k], after_twin[k], f"a substep after the decay against a fresh twin: {k}")
        a.close(), twin.close()
    finally:
        H.set_option("lookahead", None)


def test_no_hidden_state_behind_a_shape_between_two_substeps():
    """sim A: substep, shape, substep. Twin B: a fresh sim that uploads A's state as downloaded after the shape, then one substep. With the look-ahead forced, A's second
    substep would consume a memo of the velocity before the shape if apply did not forget it"""
    import hnanosolver_amd as H

    clean = {k: np.nan_to_num(np.array(v), nan=0.5, posinf=1.0, neginf=-1.0) for k, v in start_state().items()}
    H.set_option("lookahead", "1")
    try:
        g1, a = fresh_sim(clean, near_only=True)
        a.core_substep(3, DT, VS)
        assert a.lookahead_counts()[0] >= 1 and a.lookahead_counts()[1] == 0
        a.shape(DT, TURBULENCE["mixed"], {"density": (2.0, 0.0), "temperature": (1.0, 0.5)})
        mid = download(a, NAMES)
        a.core_substep(3, DT, VS)
        assert a.lookahead_counts()[1] == 0, "the second substep consumed the memo of the velocity before the shape"
        g2, b = fresh_sim(mid, near_only=True)
        b.core_substep(3, DT, VS)
        after_a, after_b = download(a, NAMES), download(b, NAMES)
        for k in after_a:
            assert_words(after_a[k], after_b[k], f"substep, shape, substep against the twin: {k}")
        assert (words(after_a["vel"]) != words(mid["vel"])).any()
        a.close(), b.close()
    finally:
        H.set_option("lookahead", None)


def test_a_strict_sub_range_leaves_the_other_leaves_alone():
    g, s = fresh_sim()
    try:
        n = g.leaf_count()
        first, count = 3, n - 7
        before = everything(s)
        g.set_active_range(first, count)
        rows = slice(first * 512, (first + count) * 512)
        check(s, before, TURBULENCE["mixed"], {"soot": (3.0, 1.0)}, "launch range", rows)
        g.set_active_range(0, n)
    finally:
        s.close()


def arena_words(sim):
    """every word of the sim's arena but the digest accumulators: vel, adv, tmp | div, p_a, p_b | cur, nxt per field | q4 (the four combustion fields are among NAMES)"""
    import torch

    unit = sim.grid.voxel_count()  # words of one float field: a multiple of 64, so the slices touch
    base = _lib.lib.hns_sim_field_ptr(sim._ptr, NAMES[0].encode()) - 12 * 4 * unit
    total = (12 + 2 * len(NAMES) + 4) * unit
    torch.cuda.synchronize()
    return torch.as_tensor(device._DeviceWords(base, total, sim), device="cuda").cpu().numpy().view(np.uint32), unit


def test_apply_late_on_a_non_blocking_stream_inside_the_arena():
    """the state arrives behind a delay on a non-blocking stream (until then the sim holds NaN): the result is the null-stream run's, and every word of the sim's arena
    outside the velocity and the decayed fields' current buffers -- adv, tmp, div, both pressure buffers, every `nxt`, q4, the other fields -- keeps its value"""
    import torch

    import stream_cases

    g, s = fresh_sim()
    try:
        n = g.voxel_count()
        nan = {"vel": np.full((n, 3), stream_cases.NAN_WORD, np.uint32).view(F), **{k: np.full(n, stream_cases.NAN_WORD, np.uint32).view(F) for k in NAMES}}
        keep = {k: torch.from_numpy(np.array(a)).pin_memory() for k, a in start_state().items()}  # pinned: hns_sim_upload's copies are asynchronous
        state = {k: t.numpy() for k, t in keep.items()}
        spec = {**TURBULENCE["mixed"], "control": "density", "control_lo": 0.25, "control_hi": 0.75}
        decay = {"density": (2.0, 0.0), "dust": (1.0, 3.0)}

        def fn(stream):
            s.upload(state, stream)
            s.shape(DT, spec, decay, stream=stream)

        s.upload(nan)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(0)
        host = time.perf_counter() - t0
        ref = everything(s)
        want = expected({**{k: np.array(v) for k, v in start_state().items()}, "div": ref["div"], "p": ref["p"]}, g.coords(), DT, spec, decay)
        for k in want:
            assert_words(ref[k], want[k], f"the null-stream run against the mirror: {k}")
        s.upload(nan)
        pre, unit = arena_words(s)
        delay = stream_cases.Delay(torch)
        stream_cases.late_call(fn, {}, {}, delay, delay.for_host_time(host), True, None, "Shaping.apply")
        got = everything(s)
        for k in ref:
            assert_words(got[k], ref[k], f"late on a non-blocking stream: {k}")
        post, _ = arena_words(s)
        written = np.zeros(len(post), bool)
        written[:3 * unit] = True  # vel
        for k in range(len(NAMES)):  # every cur: the upload writes them all
            written[(12 + 2 * k) * unit:(13 + 2 * k) * unit] = True
        bad = np.flatnonzero((pre != post) & ~written)
        assert not len(bad), f"{len(bad)} words of the arena outside vel and the fields' current buffers changed, the first at word {bad[0]} (slice {bad[0] // unit})"
    finally:
        torch.cuda.synchronize()
        s.close()


def test_refusals_that_need_objects_write_nothing(sim):
    sim.upload({k: np.array(v) for k, v in start_state().items()})
    before = everything(sim)
    spec = TURBULENCE["wide"]
    for turbulence, decay, word in (({**spec, "control": "nope"}, None, "nope"), (spec, {"nope": (1.0, 0.0)}, "nope"), (spec, {"collision_sdf": (1.0, 0.0)}, "collision_sdf"),
                                    (None, {"density": (1.0, 0.0), "vel": (1.0, 0.0)}, "vel")):
        with pytest.raises(ValueError, match=word):  # (HNS_ERR_INVALID_ARGUMENT surfaces as ValueError)
            sim.shape(DT, turbulence, decay)
    # a name given twice: through the C structs, a dict cannot hold it
    arr = (_lib.hns_decay_spec * 2)()
    for d in arr:
        d.name, d.rate, d.target = b"density", 1.0, 0.0
    with device.Shaping() as sh:
        tb = device.Shaping.turbulence_spec(spec)
        import ctypes as C

        assert _lib.lib.hns_shaping_apply(sh._ptr, sim._ptr, DT, C.byref(tb), arr, 2) == _lib.HNS_ERR_INVALID_ARGUMENT
        text = _lib.lib.hns_last_error().decode()
        assert text.startswith("hns_shaping_apply:") and "twice" in text and "density" in text
        assert _lib.lib.hns_shaping_apply(sh._ptr, None, DT, C.byref(tb), arr, 1) == _lib.HNS_ERR_INVALID_ARGUMENT and "null sim" in _lib.lib.hns_last_error().decode()
    for k, v in everything(sim).items():
        assert_words(v, before[k], f"after the refusals: {k}")


def test_a_grid_without_leaves_launches_nothing():
    from hnanosolver_amd import api

    g = api.create_grid_from_leaves(np.zeros((0, 3), np.int32), VS)
    s = device.Sim(g, ["density"])
    s.shape(DT, TURBULENCE["wide"], {"density": (1.0, 0.0)})
    import torch

    torch.cuda.synchronize()
    s.close()
