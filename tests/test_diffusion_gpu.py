"""Diffusing a device-resident sim on the GPU: hns_diffusion_apply (k_diffuse_faces, k_diffuse, k_diffuse_copy of hns_diffusion.hip) through device.Diffusion and
Sim.diffuse, against the float32 numpy mirror of tests/diffusion_cases.py, which restates include/hns.h. There is no tolerance anywhere: every float field, the velocity,
the divergence, the pressure and the masks are compared as words, on the 25-leaf fixture of diffusion_cases.fixture() -- negative origins, a lone leaf, leaves without
unknowns, a 2 x 2 x 2 block with open and wall faces across leaf planes in all six directions, every face count 0 .. 6.

Not here: the refusal of a lent sim (no call of the ABI hands one out: tests/test_shaping_gpu.py says the same of the check_sim both share), and two HIP devices."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import diffusion_cases as dc
from diag_cases import read_field
from frame_cases import download, make_sim
from hnanosolver_amd import _lib, device

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 32
DT = 0.04  # a = coefficient * DT / VS^2 = 40.96 coefficient
FLOATS = ["density", "temperature", "fuel", "waste", "flame", "soot", "heat", "dust"]
NAMES = FLOATS + ["collision_sdf"]
EIGHT = {k: c for k, c in zip(FLOATS, (0.0012, 0.012, 0.1, 0.0, 0.78, 0.004, 0.03, 1e-9))}  # a from 4e-8 to 32, one of them 0
TERMS = {
    "one field": ({"temperature": 0.012}, 0.0),
    "eight fields": (EIGHT, 0.0),
    "velocity": ({}, 0.02),
    "velocity and three fields": ({"density": 0.1, "heat": 0.0012, "soot": 0.3}, 0.05),
}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_words(got, want, what, nan_for_nan=False):
    g, w = words(got).reshape(len(got), -1), words(want).reshape(len(want), -1)
    differ = g != w
    if nan_for_nan:  # a NaN's sign and payload are the compiler's to choose (special_cases.nan_sign_differences): a NaN in the mirror must be a NaN here
        differ &= ~(np.isnan(np.asarray(got).reshape(len(got), -1)) & np.isnan(np.asarray(want).reshape(len(want), -1)))
    bad = np.flatnonzero(differ.any(1))
    assert not len(bad), f"{what}: {len(bad)} of {len(g)} voxels differ, first {bad[:4].tolist()}: {np.asarray(got)[bad[:4]].tolist()} vs {np.asarray(want)[bad[:4]].tolist()}"


@functools.lru_cache(maxsize=None)
def start_state(special=False):
    fx = dc.fixture()
    n = len(fx["origins"]) * 512
    rng = np.random.default_rng(29)
    st = {"vel": rng.standard_normal((n, 3)).astype(F)}
    for i, k in enumerate(FLOATS):
        st[k] = (rng.standard_normal(n) * (i + 1) + i).astype(F)
    st["collision_sdf"] = np.array(fx["sdf"])
    if special:  # NaN, +-inf, zeros of both signs and subnormals at 1 % each, in the fields, the velocity and the SDF
        for a in st.values():
            flat = a.reshape(-1)
            for value in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -3e-42):
                flat[rng.random(flat.size) < 0.01] = value
    for a in st.values():
        a.setflags(write=False)
    return st


def fresh_sim(state=None, masks="fixture", names=NAMES):
    fx = dc.fixture()
    st = state or start_state()
    g, s = make_sim(fx["origins"], names, {k: np.array(v) for k, v in st.items() if k == "vel" or k in names}, np.array(fx["masks"]) if masks == "fixture" else masks, VS)
    assert np.array_equal(g.coords(), dc.coords(fx["origins"]))  # the mirror's rows are the library's
    return g, s


def everything(sim, names=NAMES):
    """the velocity, every field, the divergence, the pressure buffer and the masks, as the device holds them"""
    import torch

    torch.cuda.synchronize()
    out = download(sim, names)
    n = sim.grid.leaf_count()
    out["div"] = read_field(_lib.lib.hns_sim_divergence_ptr(sim._ptr), n)
    out["p"] = read_field(_lib.lib.hns_sim_pressure_ptr(sim._ptr), n)
    out["masks"] = sim.active_masks().reshape(n, 64).view(np.uint32)
    return out


def expected(before, fields, viscosity, iterations, method, collide, threshold=0.0, active="fixture"):
    fx = dc.fixture()
    state = {k: before[k] for k in before if k not in ("div", "p", "masks")}
    out = dc.apply_mirror(fx["origins"], state, DT, VS, fields, viscosity, iterations, method, collide, threshold, fx["active"] if active == "fixture" else active, nb=fx["nb"])
    return {**before, **out}


def check(sim, before, fields, viscosity, iterations, method, collide, what, active="fixture", nan_for_nan=False, threshold=0.0):
    sim.diffuse(DT, VS, fields, viscosity=viscosity, iterations=iterations, method=method, collide=collide, threshold=threshold)
    got, want = everything(sim), expected(before, fields, viscosity, iterations, method, collide, threshold, active)
    for k in want:
        assert_words(got[k], want[k], f"{what}: {k}", nan_for_nan and k not in ("masks",))
    return got


def upload(sim, state):
    sim.upload({k: np.array(v) for k, v in state.items()})


@pytest.fixture(scope="module")
def sim():
    g, s = fresh_sim()
    yield s
    s.close()


@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("collide", [False, True])
@pytest.mark.parametrize("method", sorted(dc.METHODS))
def test_every_word_equals_the_mirror(sim, method, collide, terms):
    """iterations 1 (the copy), 2 and 3 (both parities of the ping-pong, Chebyshev's first accelerated step from b and from the scratch) and 7"""
    fields, viscosity = TERMS[terms]
    for iterations in (1, 2, 3, 7):
        upload(sim, start_state())
        before = everything(sim)
        got = check(sim, before, fields, viscosity, iterations, method, collide, f"{method}, collide {collide}, {terms}, {iterations} iterations")
        unknown = dc.classes(len(before["vel"]), dc.fixture()["active"], before["collision_sdf"], collide, 0.0)[0]
        for k, c in list(fields.items()) + ([("vel", viscosity)] if viscosity else []):
            changed = (words(got[k]) != words(before[k])).reshape(len(unknown), -1).any(1)
            assert not changed[~unknown].any(), k
            if c == 0:
                assert not changed.any(), k
            elif c * DT / VS ** 2 >= 0.01:  # (a tiny a changes only the words whose last bit it reaches)
                assert changed[unknown].mean() > 0.5, (k, changed[unknown].mean())


def test_without_masks_every_voxel_is_an_unknown():
    g, s = fresh_sim(masks=None)
    try:
        for method, collide in (("jacobi", True), ("chebyshev", False)):
            upload(s, start_state())
            before = everything(s)
            assert (before["masks"] == 0xFFFFFFFF).all()
            check(s, before, {"density": 0.1, "dust": 0.004}, 0.02, 3, method, collide, f"no masks, {method}", active=None)
    finally:
        s.close()


def test_a_one_leaf_grid_has_no_open_face_across_a_leaf_plane():
    from frame_cases import pack

    rng = np.random.default_rng(31)
    bits = rng.random((1, 512)) < 0.8
    st = {"vel": rng.standard_normal((512, 3)).astype(F), "density": rng.standard_normal(512).astype(F), "collision_sdf": (rng.standard_normal(512) + 1).astype(F)}
    origins = np.array([[-8, 16, 0]], np.int32)
    g, s = make_sim(origins, ["density", "collision_sdf"], {k: np.array(v) for k, v in st.items()}, pack(bits), VS)
    try:
        for method in sorted(dc.METHODS):
            s.upload({k: np.array(v) for k, v in st.items()})
            s.diffuse(DT, VS, {"density": 0.05}, viscosity=0.01, iterations=4, method=method, collide=True, threshold=0.25)
            got = download(s, ["density", "collision_sdf"])
            want = dc.apply_mirror(origins, st, DT, VS, {"density": 0.05}, 0.01, 4, method, True, 0.25, bits.reshape(-1))
            for k in want:
                assert_words(got[k], want[k], f"one leaf, {method}: {k}")
    finally:
        s.close()


@pytest.mark.parametrize("method", sorted(dc.METHODS))
def test_special_values_pass_through_by_the_arithmetic(sim, method):
    """a NaN in the SDF is not solid; a NaN, an inf or a subnormal in a field spreads exactly as the header's lines spread it"""
    st = start_state(True)
    assert np.isnan(st["collision_sdf"]).any() and np.isinf(st["vel"]).any() and (np.abs(st["density"][st["density"] != 0]) < 1e-38).any()
    for iterations in (1, 3):
        upload(sim, st)
        before = everything(sim)
        got = check(sim, before, {"density": 0.1, "heat": 0.0012, "soot": 0.3}, 0.05, iterations, method, True, f"special values, {method}, {iterations}", nan_for_nan=True)
        assert np.isnan(got["density"]).sum() > np.isnan(before["density"]).sum()
    upload(sim, start_state())


def test_no_result_depends_on_what_pooled_memory_held():
    """the sim's arena (its next-value, advected-velocity and vorticity buffers are the scratch) and the object's block come from the pool filled with 0x00, 0xFF and
    0x7F: a fresh object, then the same object after a smaller and after a larger call"""
    from pool_cases import under_every_fill

    def scenario():
        g, s = fresh_sim()
        try:
            out = {}
            with device.Diffusion() as d:
                for tag, fields, viscosity, iterations, method in (("fresh", {"density": 0.1}, 0.0, 1, "jacobi"), ("larger", EIGHT, 0.05, 3, "chebyshev"),
                                                                   ("smaller", {"heat": 0.03, "soot": 0.3}, 0.02, 2, "chebyshev"), ("one iteration", EIGHT, 0.05, 1, "jacobi")):
                    before = everything(s)
                    d.apply(s, DT, VS, fields, viscosity=viscosity, iterations=iterations, method=method, collide=True)
                    got, want = everything(s), expected(before, fields, viscosity, iterations, method, True)
                    for k in want:
                        assert_words(got[k], want[k], f"{tag}: {k}")
                        out[f"{tag}: {k}"] = got[k]
            return out
        finally:
            s.close()

    under_every_fill(scenario)


def test_apply_late_on_a_non_blocking_stream_gives_the_synchronous_bytes():
    """the state arrives behind a delay on a non-blocking stream (until then the sim holds NaN); the call is given the stream through stream="""
    import torch

    import stream_cases

    g, s = fresh_sim()
    try:
        n = g.voxel_count()
        nan = {"vel": np.full((n, 3), stream_cases.NAN_WORD, np.uint32).view(F), **{k: np.full(n, stream_cases.NAN_WORD, np.uint32).view(F) for k in NAMES}}
        keep = {k: torch.from_numpy(np.array(a)).pin_memory() for k, a in start_state().items()}  # pinned: hns_sim_upload's copies are asynchronous
        state = {k: t.numpy() for k, t in keep.items()}
        fields, viscosity = TERMS["velocity and three fields"]

        def fn(stream):
            s.upload(state, stream)
            s.diffuse(DT, VS, fields, viscosity=viscosity, iterations=3, method="chebyshev", collide=True, stream=stream)

        s.upload(nan)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(0)
        host = time.perf_counter() - t0
        ref = everything(s)
        want = expected({**{k: np.array(v) for k, v in start_state().items()}, "div": ref["div"], "p": ref["p"], "masks": ref["masks"]}, fields, viscosity, 3, "chebyshev", True)
        for k in want:
            assert_words(ref[k], want[k], f"the null-stream run against the mirror: {k}")
        s.upload(nan)
        torch.cuda.synchronize()
        delay = stream_cases.Delay(torch)
        stream_cases.late_call(fn, {}, {}, delay, delay.for_host_time(host), True, None, "Diffusion.apply")
        got = everything(s)
        for k in ref:
            assert_words(got[k], ref[k], f"late on a non-blocking stream: {k}")
    finally:
        torch.cuda.synchronize()
        s.close()


def clean_state():
    return {k: np.array(v) for k, v in start_state().items()}


def test_a_diffuse_that_wrote_the_velocity_is_forgotten_and_one_of_fields_alone_keeps_the_memo():
    """sim A: substep, diffuse, substep. Twin B: a fresh sim uploaded with A's state after the diffuse, then one substep. With the look-ahead forced, A's second substep
    would consume a memo of the velocity before the diffuse (which also lies in the scratch the diffuse used) if apply did not forget it; after a diffuse of fields alone
    the memo is consumed, and the substep still equals the twin's"""
    import hnanosolver_amd as H

    H.set_option("lookahead", "1")
    try:
        for viscosity, fields in ((0.02, {"density": 0.1}), (0.0, {"density": 0.1, "temperature": 0.012})):
            g1, a = fresh_sim(clean_state(), masks=None)
            a.core_substep(3, DT, VS)
            counts = a.lookahead_counts()
            assert counts[0] >= 1 and counts[1] == 0
            a.diffuse(DT, VS, fields, viscosity=viscosity, iterations=3, method="chebyshev", collide=True)
            assert a.lookahead_counts() == counts
            mid = download(a, NAMES)
            a.core_substep(3, DT, VS)
            if viscosity:
                assert a.lookahead_counts()[1] == 0, "the second substep consumed the memo of the velocity before the diffuse"
            else:
                assert a.lookahead_counts()[1] >= 1, "the memo was dropped by a call that wrote no velocity"
            g2, b = fresh_sim(mid, masks=None)
            b.core_substep(3, DT, VS)
            after_a, after_b = download(a, NAMES), download(b, NAMES)
            for k in after_a:
                assert_words(after_a[k], after_b[k], f"substep, diffuse (viscosity {viscosity}), substep against the twin: {k}")
            assert (words(after_a["vel"]) != words(mid["vel"])).any()
            a.close(), b.close()
    finally:
        H.set_option("lookahead", None)


def test_refusals_that_need_objects_write_nothing(sim):
    upload(sim, start_state())
    before = everything(sim)
    lib = _lib.lib

    def raw(d, s, rows, collide=0):
        arr = (_lib.hns_diffusion_term * len(rows))()
        for t, (name, c) in zip(arr, rows):
            t.name, t.coefficient = name, c
        sp = _lib.hns_diffusion_spec(3, 0, 0.02, collide, 0.0)
        code = lib.hns_diffusion_apply(d._ptr, None if s is None else s._ptr, DT, VS, C.byref(sp), arr, len(rows))
        return code, lib.hns_last_error().decode()

    with device.Diffusion() as d:
        for rows, word in (([(b"nope", 0.1)], "nope"), ([(b"density", 0.1), (b"collision_sdf", 0.1)], "collision_sdf"), ([(b"density", 0.1), (b"heat", 0.1), (b"density", 0.2)], "twice")):
            code, text = raw(d, sim, rows)
            assert code == _lib.HNS_ERR_INVALID_ARGUMENT and text.startswith("hns_diffusion_apply:") and word in text, text
        code, text = raw(d, None, [(b"density", 0.1)])
        assert code == _lib.HNS_ERR_INVALID_ARGUMENT and "null sim" in text
        with pytest.raises(ValueError, match="nope"):  # (the Python class, before the library)
            d.apply(sim, DT, VS, {"nope": 0.1})
        with pytest.raises(ValueError, match="collision_sdf"):  # (HNS_ERR_INVALID_ARGUMENT surfaces as ValueError)
            d.apply(sim, DT, VS, {"collision_sdf": 0.1})
        # a narrowed launch range: a face towards a leaf outside it would be neither open nor closed
        n = sim.grid.leaf_count()
        sim.grid.set_active_range(3, n - 7)
        try:
            code, text = raw(d, sim, [(b"density", 0.1)])
            assert code == _lib.HNS_ERR_INVALID_ARGUMENT and "launch range" in text, text
        finally:
            sim.grid.set_active_range(0, n)
        for k, v in everything(sim).items():
            assert_words(v, before[k], f"after the refusals: {k}")
        # collide on a sim without the field
        g2, bare = fresh_sim(names=FLOATS[:2])
        try:
            was = everything(bare, FLOATS[:2])
            code, text = raw(d, bare, [(b"density", 0.1)], collide=1)
            assert code == _lib.HNS_ERR_INVALID_ARGUMENT and "collision_sdf" in text and "collide" in text, text
            for k, v in everything(bare, FLOATS[:2]).items():
                assert_words(v, was[k], f"after collide without the field: {k}")
        finally:
            bare.close()


def test_nothing_to_do_and_a_grid_without_leaves_launch_nothing(sim):
    from hnanosolver_amd import api
    import torch

    upload(sim, start_state())
    before = everything(sim)
    sim.diffuse(DT, VS, None), sim.diffuse(0.0, VS, {"density": 0.1}, viscosity=0.5), sim.diffuse(DT, VS, {"density": 0.0, "heat": 0.0}, viscosity=0.0, collide=True)
    for k, v in everything(sim).items():
        assert_words(v, before[k], f"a call with nothing to do: {k}")
    g = api.create_grid_from_leaves(np.zeros((0, 3), np.int32), VS)
    s = device.Sim(g, ["density"])
    s.diffuse(DT, VS, {"density": 0.1}, viscosity=0.1)
    torch.cuda.synchronize()
    s.close()
