"""Point values added into fields on the GPU: hns_dev_splat_points (k_splat_points, k_splat_finish of hns_splat.hip), hns_sim_splat_points and their Python mirrors.

Every comparison is equality of bytes against the host mirror hns_grid_splat_points, which tests/test_splat.py holds to the numpy restatement of include/hns.h on the CPU:
fields, status, the rejected count, masks. There is no tolerance: the sums are integers. Grids, points, values and the conditions they meet: tests/splat_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import splat_cases as sp
from frame_cases import LAUNCH_RANGES, download, launch_range, make_sim, random_state
from pool_cases import arena_fill

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 24.0
SENTINEL = 0xAB
REJECTED_BEFORE = 5  # d_rejected is added to, not set


class Rig:
    """a device grid over a leaf set (the host mirror runs on the same grid: it fetches the host tables once)"""

    def __init__(self, origins):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.grid = api.create_grid_from_leaves(np.ascontiguousarray(origins, dtype=np.int32), VS)

    def dev(self, a):
        return self.t.from_numpy(np.array(a)).cuda()

    def padded(self, a, fill=0.0):
        """(device tensor one row longer than a, its first len(a) rows): no call gets a null pointer for n = 0, and the row behind the last is watched"""
        a = np.asarray(a)
        full = self.t.full((len(a) + 1, *a.shape[1:]), fill, dtype=self.t.float32, device="cuda")
        full[: len(a)] = self.dev(a)
        return full, full[: len(a)]

    def splat(self, fields, xyz, values, q=-32, what=""):
        """one hns_dev_splat_points call on copies -> (new fields, status, rejected); xyz, the values and the byte behind the last status are watched"""
        n = len(xyz)
        d_fields = [self.dev(f) for f in fields]
        pfull, p = self.padded(np.asarray(xyz, dtype=F).reshape(-1, 3), 7.0)
        vals = [self.padded(v, 7.0) for v in values]
        status = self.t.full((n + 1,), SENTINEL, dtype=self.t.uint8, device="cuda")
        rejected = self.t.full((1,), REJECTED_BEFORE, dtype=self.t.int64, device="cuda")
        self.D.splat_points(self.grid, d_fields, p, [v[1] for v in vals], q, status[:n], rejected)
        st = status.cpu().numpy()
        assert st[n] == SENTINEL, f"{what}: status was written behind its last byte"
        assert sp.same_bytes(pfull.cpu().numpy()[:n], np.asarray(xyz, dtype=F).reshape(-1, 3)) and (pfull.cpu().numpy()[n:] == 7.0).all(), f"{what}: xyz changed"
        for (vfull, _), v in zip(vals, values):
            assert sp.same_bytes(vfull.cpu().numpy()[:n], v) and (vfull.cpu().numpy()[n:] == 7.0).all(), f"{what}: point values changed"
        return [f.cpu().numpy() for f in d_fields], st[:n], int(rejected.cpu().numpy()[0]) - REJECTED_BEFORE

    def mirror(self, fields, xyz, values, q=-32, masks=None, activate=True):
        return sp.mirror(self.grid, fields, xyz, values, q, masks, activate)


@functools.lru_cache(maxsize=None)
def rig(name):
    sp.oracle_grid(name)  # (asserts the case's conditions)
    return Rig(sp.case(name)[0])


def assert_equal_the_mirror(R, fields, xyz, values, q, what):
    got, status, rej = R.splat(fields, xyz, values, q, what)
    want, want_status, want_rej, _ = R.mirror(fields, xyz, values, q)
    for i in range(len(fields)):
        d = np.flatnonzero(got[i].reshape(-1).view(np.uint32) != want[i].reshape(-1).view(np.uint32))
        assert len(d) == 0, f"{what}: field {i}: {len(d)} words differ, first at {d[:6].tolist()}"
        assert len(xyz) == 0 or not sp.same_bytes(got[i], fields[i]), f"{what}: field {i}: nothing was added"
    assert sp.same_bytes(status, want_status), f"{what}: status"
    assert rej == want_rej, f"{what}: rejected {rej} against {want_rej}"
    return got


# ---------------------------------------------------------------------------------------------------------------
# 1. the device equals the host mirror
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", sp.COUNTS)
@pytest.mark.parametrize("name", sp.GRIDS)
def test_device_equals_the_mirror(name, n):
    R, xyz = rig(name), sp.case(name)[3][:n]
    for label, (fields, values) in sp.channel_sets(name).items():  # float | Vec3f | 1 float + velocity (one launch) | 5 floats + velocity (two)
        assert_equal_the_mirror(R, fields, xyz, [v[:n] for v in values], -32, f"{name} n={n} {label}")


@pytest.mark.parametrize("q", sp.QUANTA)
@pytest.mark.parametrize("name", sp.GRIDS)
def test_device_equals_the_mirror_at_every_quantum(name, q):
    R, xyz = rig(name), sp.case(name)[3]
    fields, values = sp.channel_sets(name)["float+vec3"]
    assert_equal_the_mirror(R, fields, xyz, values, q, f"{name} Q={q}")


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_taps_land_in_every_leaf_whatever_the_launch_range(kind):
    """include/hns.h: a tap lands in a leaf whatever the grid's launch range, ghost leaves included -- the bytes of the whole range, which equal the mirror, under
    set_active_range on a strict inner range and under set_active_leaves(n // 2)"""
    R, xyz = rig("ragged32"), sp.case("ragged32")[3]
    fields, values = sp.channel_sets("ragged32")["float+vec3"]
    whole = assert_equal_the_mirror(R, fields, xyz, values, -32, "whole range")
    _, whole_status, whole_rejected = R.splat(fields, xyz, values, -32, "whole range")
    with launch_range(R.grid, kind):
        got, status, rejected = R.splat(fields, xyz, values, -32, kind)
    assert R.grid.active_leaves() == R.grid.leaf_count()
    for i in range(len(fields)):
        assert sp.same_bytes(got[i], whole[i]), f"{kind}: field {i} differs from the whole range's"
    assert sp.same_bytes(status, whole_status) and rejected == whole_rejected, f"{kind}: status or rejected"


def test_special_values_equal_the_mirror():
    """NaN, inf and out-of-range positions land nowhere; NaN, inf and out-of-bound values are counted and add nothing; a wrapped accumulator wraps as the mirror's"""
    R, (o, vel, phi, _, _, _, _) = rig("ragged32"), sp.case("ragged32")
    xyz = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [3e9, 1, 1], [1, -3e9, 1], [1.5, 1.5, 1.5], [1.5, 1.5, 1.5], [1.5, 1.5, 1.5], [2, 2, 2], [2.25, 2.5, 2.5]]
                   + [[3.0, 3.0, 3.0]] * 5, dtype=F)
    vals = np.array([1, 1, 1, 1, 1, np.nan, np.inf, 2.0 ** 34, -np.inf, 2.0 ** 32] + [2.0 ** 29] * 5, dtype=F)  # five terms of 2^61 quanta into one voxel
    got, status, rej = R.splat([phi[0], vel], xyz, [vals, np.stack([vals, -vals, vals], 1)], -32, "special values")
    want, want_status, want_rej, _ = R.mirror([phi[0], vel], xyz, [vals, np.stack([vals, -vals, vals], 1)], -32)
    assert sp.same_bytes(got[0], want[0]) and sp.same_bytes(got[1], want[1]) and sp.same_bytes(status, want_status)
    assert status.tolist() == [0] * 5 + [8] * 10 and rej == want_rej == 4 * 8 * 4


# ---------------------------------------------------------------------------------------------------------------
# 2. contention, reproducibility, shared calls
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ("one_cell", "random"))
def test_contended_sums_are_the_same_bytes_twice_and_equal_the_mirror(kind):
    R, (o, vel, phi, _, _, _, _) = rig("dense32"), sp.case("dense32")
    rng = np.random.default_rng(17)
    if kind == "one_cell":  # 4,096 points in one cell: 4,096 terms into each of eight voxels, per channel
        xyz = (np.array([13.0, 7.0, 22.0]) + rng.uniform(0.0, 1.0, (4096, 3))).astype(F)
    else:  # 2^17 points over 32^3 voxels: four to a voxel on average
        xyz = rng.uniform(-1.0, 33.0, (2 ** 17, 3)).astype(F)
    vals, vvals = (rng.standard_normal(len(xyz)) * 3.0).astype(F), (rng.standard_normal((len(xyz), 3)) * 3.0).astype(F)
    first = assert_equal_the_mirror(R, [phi[0], vel], xyz, [vals, vvals], -32, kind)
    second, _, _ = R.splat([phi[0], vel], xyz, [vals, vvals], -32, kind)
    assert sp.same_bytes(first[0], second[0]) and sp.same_bytes(first[1], second[1]), f"{kind}: two runs differ"


def test_output_i_of_a_shared_call_equals_a_call_with_field_i_alone():
    R, xyz = rig("sparse_far"), sp.case("sparse_far")[3]
    fields, values = sp.channel_sets("sparse_far")["5float+vec3"]
    together, _, _ = R.splat(fields, xyz, values)
    for i in range(len(fields)):
        alone, _, _ = R.splat([fields[i]], xyz, [values[i]])
        assert sp.same_bytes(alone[0], together[i]), f"field {i}"


# ---------------------------------------------------------------------------------------------------------------
# 3. the accumulator between calls
# ---------------------------------------------------------------------------------------------------------------


def a_then_b(R, name):
    """splat A (one channel: a fresh accumulator is made for one), then B into A's result (eight channels, other points: the accumulator grows to four and runs two
    launches), then A's points again with two fields (four channels)"""
    o, vel, phi, xyz, vals, vvals, _ = sp.case(name)
    half = len(xyz) // 2
    got_a, _, _ = R.splat([phi[0]], xyz[:half], [vals[0][:half]])
    want_a = R.mirror([phi[0]], xyz[:half], [vals[0][:half]])[0]
    vb = [vals[1][half:], vals[2][half:], vals[3][half:], vals[4][half:], vals[5][half:], vvals[half:]]
    got_b, _, _ = R.splat([got_a[0], phi[1], phi[2], phi[3], phi[4], vel], xyz[half:], vb)
    want_b = R.mirror([want_a[0], phi[1], phi[2], phi[3], phi[4], vel], xyz[half:], vb)[0]
    got_c, _, _ = R.splat([got_b[0], got_b[5]], xyz[:half], [vals[2][:half], vvals[:half]])
    want_c = R.mirror([want_b[0], want_b[5]], xyz[:half], [vals[2][:half], vvals[:half]])[0]
    for got, want, what in ((got_a, want_a, "A"), (got_b, want_b, "A then B"), (got_c, want_c, "A then B then C")):
        for i in range(len(got)):
            assert sp.same_bytes(got[i], want[i]), f"{name}: {what}: field {i}"
    return np.concatenate([got_c[0], got_c[1].reshape(-1)])


@pytest.mark.parametrize("name", ("ragged32", "dense32"))
def test_a_second_call_starts_from_a_clean_accumulator(name):
    R = rig(name)
    R.grid.release_cache()  # (whatever accumulator earlier tests left with the grid)
    plain = a_then_b(R, name)
    for fill in (255, 127):  # a fresh accumulator drawn from a pool that hands out NaN / 3.39e38 / -1 bytes
        R.grid.release_cache()
        with arena_fill(fill):
            assert sp.same_bytes(a_then_b(R, name), plain), f"{name}: arena_fill {fill}"
    R.grid.release_cache()
    assert sp.same_bytes(a_then_b(R, name), plain), f"{name}: after hns_grid_release_cache"


def test_no_points_look_at_no_device_pointer():
    from hnanosolver_amd import _lib

    R, lib = rig("one_leaf"), _lib.load_library()
    bogus = (C.c_void_p * 2)(0x10, None)
    assert lib.hns_dev_splat_points(R.grid.ptr, bogus, (C.c_int * 2)(1, 3), 2, None, bogus, 0, -32, 0x10, 0x10, None) == 0
    R.t.cuda.synchronize()
    phi = sp.case("one_leaf")[2][0]
    got, status, rej = R.splat([phi], np.zeros((0, 3), F), [np.zeros(0, F)])
    assert sp.same_bytes(got[0], phi) and len(status) == 0 and rej == 0


# ---------------------------------------------------------------------------------------------------------------
# 4. Sim.splat
# ---------------------------------------------------------------------------------------------------------------

SIM_NAMES = ["density", "fuel", "collision_sdf"]


@pytest.mark.parametrize("activate,with_masks", ((True, True), (False, True), (True, False)))
def test_sim_splat_equals_the_mirror_on_the_downloaded_sim(activate, with_masks):
    import torch

    from hnanosolver_amd import api

    o, _, _, xyz, vals, vvals, masks = sp.case("ragged32")
    state = random_state(13, len(o), SIM_NAMES)
    m0 = np.array(masks) if with_masks else None
    (g, s), (g2, twin) = make_sim(o, SIM_NAMES, state, m0, VS), make_sim(o, SIM_NAMES, state, m0, VS)
    for sim in (s, twin):
        for _ in range(2):  # (two core substeps with one dt: the second looks ahead, its memo is pending)
            sim.core_substep(3, 0.04, VS)
    assert s.substep_plan()["advect_vector"] == "memo" and s.lookahead_counts()[0] >= 1
    now, m_now = download(s, SIM_NAMES), (s.active_masks() if with_masks else None)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    p = dev(xyz)

    # float fields only: the velocity is not written and the memo stays
    st = s.splat({"fuel": dev(vals[0]), "density": dev(vals[1])}, p, activate=activate, status=True)
    assert s.substep_plan()["advect_vector"] == "memo", "a splat into float fields dropped the look-ahead memo"
    want, want_status, _, want_masks = sp.mirror(g, [now["fuel"], now["density"]], xyz, [vals[0], vals[1]], -32, m_now, activate)
    assert sp.same_bytes(st.cpu().numpy(), want_status)
    # then the velocity: the memo goes
    assert s.splat({"density": dev(vals[2])}, p, velocity=dev(vvals), log2_quantum=-24, activate=activate) is None
    assert s.substep_plan()["advect_vector"] != "memo", "a splat into the velocity kept the look-ahead memo"
    want2, _, _, want_masks = sp.mirror(g, [want[1], now["vel"]], xyz, [vals[2], vvals], -24, want_masks, activate)
    expect = {"vel": want2[1], "density": want2[0], "fuel": want[0], "collision_sdf": now["collision_sdf"]}
    after = download(s, SIM_NAMES)
    for k in expect:
        assert sp.same_bytes(after[k], expect[k]), f"Sim.splat: {k}"
    if with_masks:
        assert sp.same_bytes(s.active_masks(), want_masks) and sp.same_bytes(want_masks, m_now) == (not activate)
    else:
        assert (s.active_masks() == 0xFF).all(), "a sim with NULL masks stays all-active"

    # the frame goes on: a substep, the deactivation and a regrid equal the same sequence on a twin uploaded with the mirror's result
    twin.upload(expect)
    if with_masks:
        twin.set_active_masks(want_masks)
    for sim in (s, twin):
        sim.core_substep(3, 0.04, VS)
        sim.deactivate({"density": 0.5}, velocity=0.5)
    keep = [s.regrid(1), twin.regrid(1)]
    assert np.array_equal(keep[0].coords(), keep[1].coords())
    a, b = download(s, SIM_NAMES), download(twin, SIM_NAMES)
    for k in a:
        assert sp.same_bytes(a[k], b[k]), f"after substep, deactivate and regrid: {k}"
    assert sp.same_bytes(s.active_masks(), twin.active_masks())
    # and the calls work on the new grid
    o2 = np.ascontiguousarray(s.grid.coords()[::512], dtype=np.int32)
    m2 = s.active_masks()
    s.splat({"fuel": dev(vals[3])}, p, activate=activate)
    want3, _, _, want_m3 = sp.mirror(s.grid, [a["fuel"]], xyz, [vals[3]], -32, m2, activate)
    assert sp.same_bytes(download(s, SIM_NAMES)["fuel"], want3[0]) and sp.same_bytes(s.active_masks(), want_m3) and len(o2) == keep[0].leaf_count()


def test_refusals_come_before_anything_is_launched():
    import torch

    from hnanosolver_amd import _lib

    lib = _lib.load_library()
    o, _, _, xyz, vals, vvals, masks = sp.case("one_leaf")
    state = random_state(3, len(o), SIM_NAMES)
    g, s = make_sim(o, SIM_NAMES, state, np.array(masks), VS)
    n = 64
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    p, v, vv, field = dev(xyz[:n]), dev(vals[0][:n]), dev(vvals[:n]), dev(state["density"])
    status = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    P = lambda *ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    N = lambda *names: (C.c_char_p * len(names))(*names)
    sim = lambda names, k, velocity, values, q=-32: lib.hns_sim_splat_points(s._ptr, names, k, velocity, p.data_ptr(), values, n, q, 1, status.data_ptr(), None, None)
    grid = lambda fields, nc, k, values, q=-32, x=p.data_ptr(): lib.hns_dev_splat_points(g.ptr, fields, (C.c_int * len(nc))(*nc), k, x, values, n, q, status.data_ptr(),
                                                                                         None, None)
    rows = [
        ("hns_sim_splat_points", lambda: sim(N(b"smoke"), 1, None, P(v)), "no float field named 'smoke'"),
        ("hns_sim_splat_points", lambda: sim(N(b"density", b"density"), 2, None, P(v, v)), "listed twice"),
        ("hns_sim_splat_points", lambda: sim(N(b"collision_sdf"), 1, None, P(v)), "collision_sdf"),
        ("hns_sim_splat_points", lambda: sim(None, 0, None, None), "nothing to write"),
        ("hns_sim_splat_points", lambda: sim(N(b"density"), 1, vv.data_ptr(), P(v), -41), "log2_quantum is -41"),
        ("hns_sim_splat_points", lambda: sim(N(b"density"), 1, None, P(None)), "values[0] is null"),
        ("hns_sim_splat_points", lambda: lib.hns_sim_splat_points(None, N(b"density"), 1, None, p.data_ptr(), P(v), n, -32, 1, None, None, None), "null sim"),
        ("hns_dev_splat_points", lambda: grid(P(field, field), (1, 1), 2, P(v, v)), "fields[1] is fields[0]"),
        ("hns_dev_splat_points", lambda: grid(P(field), (1,), 1, P(field)), "fields[0] is values[0]"),
        ("hns_dev_splat_points", lambda: grid(P(field), (1,), 1, P(v), x=field.data_ptr()), "fields[0] is xyz"),
        ("hns_dev_splat_points", lambda: grid(P(status), (1,), 1, P(v)), "fields[0] is status"),
        ("hns_dev_splat_points", lambda: grid(P(field), (2,), 1, P(v)), "ncomp[0] is 2"),
        ("hns_dev_splat_points", lambda: grid(P(field), (1,), 9, P(v)), "n_fields is 9"),
        ("hns_dev_splat_points", lambda: grid(P(field), (1,), 1, P(v), 1), "log2_quantum is 1"),
        ("hns_dev_splat_points", lambda: lib.hns_dev_splat_points(None, P(field), (C.c_int * 1)(1), 1, p.data_ptr(), P(v), n, -32, None, None, None), "null grid"),
    ]
    wrong = []
    for i, (call, fn, word) in enumerate(rows):
        code, text = fn(), lib.hns_last_error().decode()
        if code != _lib.HNS_ERR_INVALID_ARGUMENT or not text.startswith(call + ":") or word not in text:
            wrong.append(f"row {i} {call} (expects {word!r}): got {code} {text!r}")
    torch.cuda.synchronize()
    assert not wrong, "\n".join(wrong)
    assert (status.cpu().numpy() == SENTINEL).all() and sp.same_bytes(field.cpu().numpy(), state["density"])
    after = download(s, SIM_NAMES)
    for k in after:
        assert sp.same_bytes(after[k], state[k]), k
    assert sp.same_bytes(s.active_masks(), masks)
