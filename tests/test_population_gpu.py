"""Birth and death of points on the GPU: device.PointPopulation (hns_point_population_*: the count, scan, place and row kernels of hns_population.hip) against the host
mirror leafio.birth_points and the restatement of tests/population_cases.py, which tests/test_population.py holds to each other. Every comparison is equality of bytes:
a stable selection and a birth in voxel order are unique. The tile and scan boundaries come from the constants the Python layer exposes."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import order_cases as oc
import pool_cases
import population_cases as P
import stream_cases as sc
from frame_cases import LAUNCH_RANGES, download, launch_range, make_sim, random_masks, random_state
from hnanosolver_amd import _lib, api, device, fields, leafio
from hnanosolver_amd._lib import lib

pytestmark = pytest.mark.gpu

F, U32 = np.float32, np.uint32
T, S = device.POINT_POPULATION_TILE, device.POINT_POPULATION_SCAN_TILES
BAD = _lib.HNS_ERR_INVALID_ARGUMENT
VS = 1.0 / 24.0


def torch():
    import torch as t

    return t


@functools.lru_cache(maxsize=None)
def dev_grid(name):
    return api.create_grid_from_leaves(P.origins(name), VS)


def to_dev(a):
    return torch().from_numpy(np.array(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(U32).copy()


def same_words(a, b):
    t = torch()
    return a.shape == b.shape and bool(t.equal(a.contiguous().view(t.int32), b.contiguous().view(t.int32)))


# ---- select and compact ----------------------------------------------------------------------------------------------------------------------------------------------------

PATTERNS = ("all", "none", "first", "last", "alternating", "wave_edges", "random", "levels")
COUNTS = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, S * T + 1)


def make_flags(kind, n):
    """-> (flags uint8, at_least)"""
    f = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "first":
        f[:1] = 255
    elif kind == "last":
        f[n - 1:] = 1
    elif kind == "alternating":
        f[::2] = 1
    elif kind == "wave_edges":
        f[[i for i in (63, 64, 127, 128) if i < n]] = 3
    elif kind == "random":
        f = (np.random.default_rng([n, 1]).random(n) < 0.5).astype(np.uint8)
    elif kind == "levels":
        return np.random.default_rng([n, 2]).integers(0, 9, n).astype(np.uint8), 8
    return f, 1


def expected_slot(flags, at_least):
    """the restated select on the device, with torch's cumsum: -> (slot int32 with -1 for a dropped point, keep, live)"""
    t = torch()
    keep = flags >= at_least
    below = t.cumsum(keep.to(t.int64), 0) - keep.to(t.int64)
    return t.where(keep, below, t.full_like(below, -1)).to(t.int32), keep, int(keep.sum())


@pytest.mark.parametrize("n", COUNTS, ids=[str(n) for n in COUNTS])
def test_select_and_compact(n):
    t = torch()
    grid = dev_grid("one_leaf")
    pop = device.PointPopulation(grid, n)
    extra = 7
    rng = np.random.default_rng(n)
    srcs = {rb: to_dev(rng.integers(0, 2 ** 32, (n, rb // 4), dtype=np.uint64).astype(U32).view(np.int32)) for rb in (4, 12, 64)}  # any words, NaN patterns included
    srcs[4] = srcs[4].reshape(n)
    for kind in PATTERNS:
        flags_h, at_least = make_flags(kind, n)
        flags = to_dev(flags_h)
        assert pop.select(flags, at_least) is pop
        want_slot, keep, live = expected_slot(flags, at_least)
        what = f"n {n} {kind}"
        assert pop.counts() == (live, live), what
        assert same_words(pop.slot, want_slot), f"{what}: slot"
        if n <= 3 * T + 5:  # the numpy restatement, where it is cheap
            slot_h, live_h = P.restate_select(flags_h, at_least)
            assert live_h == live and np.array_equal(u32(pop.slot), slot_h), what
        for rb, src in srcs.items():
            for fill in (None, 0x7FC00000 if rb == 12 else 0xFEEDF00D):
                dst = t.empty((n + extra,) + tuple(src.shape[1:]), dtype=t.int32, device="cuda")
                sc.sentinel(dst)
                want = dst.clone()
                want[:live] = src[keep]
                if fill is not None:
                    want[live:n] = sc._signed(fill)
                assert pop.compact(src, dst, fill=fill) is dst
                assert same_words(dst, want), f"{what}: rows of {rb} bytes, fill {fill}"
                if n <= 65:
                    before = np.full((n + extra, rb // 4), sc.OUT_WORD, dtype=U32)
                    assert np.array_equal(u32(dst).reshape(n + extra, rb // 4), P.restate_compact(u32(src).reshape(n, rb // 4), before, flags_h, at_least, fill)), what
        assert u32(flags.to(t.int32)).tobytes() == flags_h.astype(np.int32).tobytes(), f"{what}: flags were written"
        if n:
            made = pop.compact(srcs[12])  # (a destination made by the call: n rows, of which live are defined)
            assert tuple(made.shape) == (n, 3) and same_words(made[:live], srcs[12][keep])
    again = np.random.default_rng(n)
    for rb in (4, 12, 64):
        fresh = again.integers(0, 2 ** 32, (n, rb // 4), dtype=np.uint64).astype(U32)
        assert u32(srcs[rb]).tobytes() == fresh.tobytes(), f"n {n}: src of {rb}-byte rows was written"
    pop.close()


def test_a_second_select_with_a_smaller_and_then_a_larger_n():
    grid = dev_grid("one_leaf")
    cap = 2 * T + 77
    pop = device.PointPopulation(grid, cap)
    rows = to_dev(np.arange(cap * 3, dtype=np.int32).reshape(cap, 3))
    for n, kind in ((cap, "random"), (65, "alternating"), (0, "all"), (T + 1, "levels"), (cap, "wave_edges")):
        flags_h, at_least = make_flags(kind, n)
        pop.select(to_dev(flags_h), at_least)
        slot_h, live = P.restate_select(flags_h, at_least)
        assert pop.counts() == (live, live) and np.array_equal(u32(pop.slot), slot_h), (n, kind)
        dst = torch().full((cap, 3), -5, dtype=torch().int32, device="cuda")
        pop.compact(rows, dst, fill=9)
        want = P.restate_compact(u32(rows), np.full((cap, 3), -5, dtype=np.int32), flags_h, at_least, 9)
        assert np.array_equal(u32(dst).reshape(cap, 3), want), (n, kind)
    pop.close()


# ---- birth ---------------------------------------------------------------------------------------------------------------------------------------------------------------------


def device_birth(pop, call, rows, start, fill, spec, voxel=True):
    """one birth into sentinel rows, behind set_live(start) when start > 0 -> (xyz, voxel, live, wanted) on the host"""
    sx, sv = P.sentinels(rows)
    x, v = to_dev(sx), to_dev(sv.view(np.int32))
    if start:
        pop.set_live(start)
    call(x, v if voxel else None, append=start > 0, fill=fill, **spec)
    live, wanted = pop.counts()
    return x.cpu().numpy(), u32(v), live, wanted


@pytest.mark.parametrize("kind", P.FIELDS)
@pytest.mark.parametrize("grid_name", P.GRIDS)
def test_birth_matches_the_mirror(grid_name, kind):
    """the device form, and birth_sim with and without the sim's masks, on every capacity case"""
    o, grid, host = P.origins(grid_name), dev_grid(grid_name), P.host_grid(grid_name)
    v, m, spec = P.case(grid_name, kind)
    c = P.counts(o, v, m, spec["threshold"], spec["rate"], spec["max_per_voxel"], spec["seed"])[0]
    field, masks = to_dev(v), (None if m is None else to_dev(m))
    pop = device.PointPopulation(grid, 16)  # (the rows of a birth are the caller's: the capacity bounds select only)
    names = ["flame", "density"]
    state = random_state(3, len(o), names)
    state["flame"] = np.array(v)
    sim_grid, sim = make_sim(o, names, state, None if m is None else np.array(m), VS)
    sim_pop = sim.point_population(0)
    for name, (rows, start, fill) in P.capacities(c).items():
        what = f"{grid_name} {kind} {name}"
        want = leafio.birth_points(host, v, m, **spec, fill=fill, start=start, capacity_rows=rows, xyz=P.sentinels(rows)[0], voxel=P.sentinels(rows)[1])
        P.same_birth(device_birth(pop, lambda x, vox, **k: pop.birth(field, x, masks, vox, **k), rows, start, fill, spec), want, what + " (device form)")
        P.same_birth(device_birth(sim_pop, lambda x, vox, **k: sim.birth(sim_pop, "flame", x, vox, use_masks=True, **k), rows, start, fill, spec), want, what + " (sim, masks)")
        bare = leafio.birth_points(host, v, None, **spec, fill=fill, start=start, capacity_rows=rows, xyz=P.sentinels(rows)[0], voxel=P.sentinels(rows)[1])
        P.same_birth(device_birth(sim_pop, lambda x, vox, **k: sim.birth(sim_pop, "flame", x, vox, use_masks=False, **k), rows, start, fill, spec), bare, what + " (sim, no masks)")
    rows = int(c.sum()) + 3  # without a voxel array, and from a field that is not 16-byte aligned
    want = leafio.birth_points(host, v, m, **spec, capacity_rows=rows, xyz=P.sentinels(rows)[0])
    odd = torch().empty(len(v) + 1, dtype=torch().float32, device="cuda")[1:]
    odd.copy_(field)
    assert odd.data_ptr() % 16 == 4
    for f in (field, odd):
        got = device_birth(pop, lambda x, vox, **k: pop.birth(f, x, masks, vox, **k), rows, 0, True, spec, voxel=False)
        assert got[0].view(U32).tobytes() == want[0].view(U32).tobytes() and got[2:] == want[2:] and (got[1] == P.VOXEL_SENTINEL).all()
    assert u32(field).tobytes() == np.asarray(v).view(U32).tobytes(), "the field was written"
    pop.close(), sim_pop.close(), sim.close()


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_every_leaf_bears_whatever_the_launch_range(kind):
    """include/hns.h: every leaf bears whatever the grid's launch range, ghost leaves included -- the device form and the sim's form under set_active_range on a strict
    inner range and under set_active_leaves(n // 2) give the rows, voxels and counts of the whole range, which equal the mirror"""
    o, grid, host = P.origins("ragged32"), dev_grid("ragged32"), P.host_grid("ragged32")
    rng = np.random.default_rng(32)
    v = rng.uniform(-0.5, 2.0, len(o) * 512).astype(F)
    m = np.packbits((rng.random((len(o), 512)) < 0.5).reshape(len(o), 64, 8), axis=2, bitorder="little").reshape(len(o), 64)
    spec = dict(P.SPEC)
    rows = leafio.birth_points(host, v, m, **spec, capacity_rows=0)[3] + 5
    want = leafio.birth_points(host, v, m, **spec, fill=True, start=0, capacity_rows=rows, xyz=P.sentinels(rows)[0], voxel=P.sentinels(rows)[1])
    field, masks = to_dev(v), to_dev(m)
    pop = device.PointPopulation(grid, 16)
    sim_grid, sim = make_sim(o, ["flame"], {"vel": np.zeros((len(o) * 512, 3), dtype=F), "flame": v}, m, VS)
    sim_pop = sim.point_population(0)
    forms = {"device form": (pop, lambda x, vox, **k: pop.birth(field, x, masks, vox, **k)), "sim": (sim_pop, lambda x, vox, **k: sim.birth(sim_pop, "flame", x, vox, use_masks=True, **k))}
    for form, (p, call) in forms.items():
        whole = device_birth(p, call, rows, 0, True, spec)
        P.same_birth(whole, want, f"whole range ({form})")
        with launch_range(p.grid, kind):
            got = device_birth(p, call, rows, 0, True, spec)
        assert p.grid.active_leaves() == len(o)
        P.same_birth(got, whole, f"{kind} ({form})")
        leaves = set((got[1][: got[2]] // 512).tolist())
        assert {0, len(o) - 1} <= leaves and len(leaves) == len(o)  # (the leaves outside either range bore too)
    pop.close(), sim_pop.close(), sim.close()


def test_birth_across_the_scan_round_on_a_128_cube():
    """4096 leaves are exactly 1024 tiles: one leaf more crosses the scan's round. One float field of 8 MB"""
    o = np.ascontiguousarray(np.concatenate([fields.dense_leaves(128), [[128, 0, 0]]]), dtype=np.int32)
    assert len(o) == 4 * S + 1
    grid, host = api.create_grid_from_leaves(o, VS), api.create_grid_from_leaves(o, VS, _lib.HNS_GRID_HOST_ONLY)
    v = np.random.default_rng(128).uniform(-0.5, 2.0, len(o) * 512).astype(F)
    v[-512:] = 1.9  # the leaf behind the round bears
    spec = dict(P.SPEC)
    pop = device.PointPopulation(grid, 0)
    wanted = leafio.birth_points(host, v, **spec, capacity_rows=0)[3]
    assert wanted > 3_000_000
    field = to_dev(v)
    for rows in (wanted, wanted - 1000):
        want = leafio.birth_points(host, v, **spec, capacity_rows=rows)
        x, vox = torch().empty((rows, 3), device="cuda"), torch().empty(rows, dtype=torch().int32, device="cuda")
        pop.birth(field, x, None, vox, **spec)
        assert pop.counts() == (want[2], want[3]) == (rows, wanted)
        assert x.cpu().numpy().view(U32).tobytes() == want[0].view(U32).tobytes() and u32(vox).tobytes() == want[1].tobytes()
        assert rows != wanted or int(want[1][-1]) == len(o) * 512 - 1  # (the leaf behind the scan's round bears the last rows)
    pop.close()
    grid.reset()


def test_append_after_a_select_and_after_set_live():
    grid_name = "ragged32_off_origin"
    o, grid, host = P.origins(grid_name), dev_grid(grid_name), P.host_grid(grid_name)
    v, m, spec = P.case(grid_name, "random")
    n = T + 300
    flags_h, at_least = make_flags("random", n)
    kept = int(flags_h.sum())
    pop = device.PointPopulation(grid, n)
    rows = n + 200  # (a compact's dst has the n rows of its select: the host does not know how many are kept)
    old = np.random.default_rng(5).uniform(90, 130, (n, 3)).astype(F)
    x0, x1 = to_dev(old), torch().full((rows, 3), 7.0, device="cuda")
    vox = torch().full((rows,), 7, dtype=torch().int32, device="cuda")
    pop.select(to_dev(flags_h), at_least).compact(x0, x1)
    pop.birth(to_dev(v), x1, None, vox, append=True, **spec)
    init_x = np.full((rows, 3), 7.0, dtype=F)
    init_x[:kept] = old[flags_h >= at_least]
    want = leafio.birth_points(host, v, **spec, start=kept, capacity_rows=rows, xyz=init_x, voxel=np.full(rows, 7, dtype=U32))
    assert want[3] > rows  # the births do not all fit: a prefix survives
    P.same_birth((x1.cpu().numpy(), u32(vox), *pop.counts()), want, "append after select")
    pop.set_live(5)
    assert pop.counts() == (5, 5)
    x2 = torch().full((rows, 3), 7.0, device="cuda")
    pop.birth(to_dev(v), x2, None, None, append=True, fill=False, **spec)
    want = leafio.birth_points(host, v, **spec, fill=False, start=5, capacity_rows=rows, xyz=np.full((rows, 3), 7.0, dtype=F))
    assert x2.cpu().numpy().view(U32).tobytes() == want[0].view(U32).tobytes() and pop.counts() == want[2:]
    pop.close()


# ---- a frame loop without a host wait ------------------------------------------------------------------------------------------------------------------------------------------


def run_frames(ask):
    """three frames -- emit, trace, select, compact of xyz and of one attribute, birth from "flame", splat --; ask: read counts() after every step and slice to the live rows"""
    t = torch()
    names, vs, cap = ["density", "flame"], 1.0 / 32, 5000  # (the third frame's births do not all fit)
    o = np.ascontiguousarray(oc.origins("ragged32"))
    state = random_state(11, len(o), names)
    state["vel"] *= F(0.3)
    _, sim = make_sim(o, names, state, random_masks(12, len(o)), vs)
    first = np.random.default_rng(13).uniform(-20, 20, (900, 3)).astype(F)
    xyz, other = t.full((cap, 3), float("nan"), device="cuda"), t.full((cap, 3), float("nan"), device="cuda")
    val, other_val = t.zeros(cap, device="cuda"), t.zeros(cap, device="cuda")
    xyz[:900] = to_dev(first)
    val[:900] = to_dev(np.random.default_rng(14).random(900).astype(F))
    live = 900
    pop = None
    for frame in range(3):
        n = live if ask else cap
        sim.emit({"density": val[:n]}, xyz[:n], padding=1)
        pop = sim.point_population(cap)
        asked = [pop.counts()] if ask else []  # form B asks behind every step; only select and birth change the answer
        status = sim.trace(xyz[:n], dt=0.05, voxel_size=vs, order=2, steps=2, status=True)
        asked += [pop.counts()] if ask else []
        pop.select(status)
        asked += [pop.counts()] if ask else []
        pop.compact(xyz[:n], other, fill=float("nan"))
        asked += [pop.counts()] if ask else []
        pop.compact(val[:n], other_val, fill=0.5)
        if ask:
            live = pop.counts()[0]
            assert asked == [(0, 0), (0, 0), (live, live), (live, live)] and live <= n
            other[live:] = float("nan")  # (what form A's fill leaves in its rows behind n: form B's arrays end at live, so nothing reads these)
            other_val[live:] = 0.5
        xyz, other, val, other_val = other, xyz, other_val, val
        sim.birth(pop, "flame", xyz, threshold=1.5, rate=0.9, max_per_voxel=3, seed=40 + frame, append=True, fill=True)
        if ask:
            live = pop.counts()[0]
        n = live if ask else cap
        sim.splat({"density": val[:n]}, xyz[:n], activate=True)
        assert not ask or pop.counts()[0] == live
    live, wanted = pop.counts()
    out = {"live": live, "wanted": wanted, "xyz": u32(xyz[:live]), "val": u32(val[:live]), "masks": sim.active_masks(), "origins": sim.grid.coords()[::512].copy()}
    out.update({"field_" + k: a for k, a in download(sim, names).items()})
    sim.close()
    return out


def test_no_host_wait_changes_nothing():
    a, b = run_frames(ask=False), run_frames(ask=True)
    print(f"live {a['live']}, wanted {a['wanted']}")
    assert a["live"] == 5000 < a["wanted"]
    assert a.keys() == b.keys()
    for k in a:
        assert pool_cases.as_bytes(a[k]) == pool_cases.as_bytes(b[k]), f"form A (n = capacity, no count read) and form B (counts() after every step) differ in {k}"
    assert not np.isnan(a["xyz"].view(F)).any()


# ---- pool and stream ----------------------------------------------------------------------------------------------------------------------------------------------------------


def test_results_do_not_depend_on_what_pooled_memory_held():
    grid_name = "ragged32_off_origin"
    grid, host = dev_grid(grid_name), P.host_grid(grid_name)
    v, m, spec = P.case(grid_name, "masked")
    n = 2 * T + 9
    flags_h, at_least = make_flags("levels", n)
    rows_h = np.random.default_rng(2).standard_normal((n, 3)).astype(F)
    want_slot, live = P.restate_select(flags_h, at_least)
    want = leafio.birth_points(host, v, m, **spec, start=live, capacity_rows=live + 500, xyz=np.zeros((live + 500, 3), dtype=F), voxel=np.zeros(live + 500, dtype=U32))

    def scenario():
        pop = device.PointPopulation(grid, n + 1000)  # drawn from the pool under the fill
        assert pop.counts() == (0, 0)
        pop.select(to_dev(flags_h), at_least)
        slot = u32(pop.slot)
        assert np.array_equal(slot, want_slot)
        dst = pop.compact(to_dev(rows_h), torch().zeros((n, 3), device="cuda"), fill=float("nan"))
        x, vox = torch().zeros((live + 500, 3), device="cuda"), torch().zeros(live + 500, dtype=torch().int32, device="cuda")
        pop.birth(to_dev(v), x, to_dev(m), vox, append=True, **spec)
        got = (x.cpu().numpy(), u32(vox), *pop.counts())
        P.same_birth(got, want, "under a fill")
        pop.close()
        return {"slot": slot, "rows": u32(dst), "xyz": got[0], "voxel": got[1], "counts": got[2:]}

    pool_cases.under_every_fill(scenario)


def test_select_compact_and_birth_late_on_a_non_blocking_stream():
    t = torch()
    grid_name = "dense64"
    grid, host = dev_grid(grid_name), P.host_grid(grid_name)
    v, _, spec = P.case(grid_name, "random")
    n = 3 * T + 5
    flags_h, at_least = make_flags("random", n)
    rows_h = np.random.default_rng(3).standard_normal((n, 4)).astype(F)
    want_slot, live = P.restate_select(flags_h, at_least)
    births = leafio.birth_points(host, v, **spec, capacity_rows=0)[3]
    cap_rows = births - 100
    want = leafio.birth_points(host, v, **spec, capacity_rows=cap_rows)
    pop = device.PointPopulation(grid, n)
    flags, rows, field = to_dev(flags_h), to_dev(rows_h), to_dev(v)
    slab = sc.Slab(t, {"dst": ((n + 3, 4), F), "xyz": ((cap_rows, 3), F), "voxel": ((cap_rows,), np.int32)}, device="cuda")
    dst, x, vox = slab.views.dst, slab.views.xyz, slab.views.voxel

    def kill(stream):
        pop.select(flags, at_least, stream=stream)
        pop.compact(rows, dst, fill=float("nan"))
        return {"slot": pop.slot}

    def bear(stream):
        pop.birth(field, x, None, vox, stream=stream, **spec)
        return {}

    delay = sc.Delay(t)
    for call, inputs, outputs, name in ((kill, {"flags": (flags, flags_h), "rows": (rows, rows_h)}, {"dst": dst}, "select + compact"),
                                        (bear, {"field": (field, np.asarray(v))}, {"xyz": x, "voxel": vox}, "birth")):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        call(0)  # the null stream, device idle before and after: also loads the code objects
        host_time = time.perf_counter() - t0
        t.cuda.synchronize()
        late = sc.late_call(call, {k: sc.Operand(d, to_dev(h)) for k, (d, h) in inputs.items()}, outputs, delay, delay.for_host_time(host_time), what=name)
        assert late.armed_held
        sc.assert_inputs_unchanged(late.inputs, {k: h for k, (d, h) in inputs.items()}, what=name)
        slab.check(name)
        if call is kill:
            assert np.array_equal(u32(late.outputs["slot"]), want_slot) and pop.counts() == (live, live)
            got = u32(late.outputs["dst"]).reshape(n + 3, 4)
            assert np.array_equal(got, P.restate_compact(rows_h, np.full((n + 3, 4), sc.OUT_WORD, dtype=U32), flags_h, at_least, P.NAN_WORD))
        else:
            P.same_birth((late.outputs["xyz"].cpu().numpy(), u32(late.outputs["voxel"]), *pop.counts()), want, name)
    pop.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------------------


def _refused(code, *fragments):
    text = lib.hns_last_error().decode()
    assert code == BAD, (code, text)
    for f in fragments:
        assert f in text, text


def test_refusals_touch_nothing():
    t = torch()
    grid = dev_grid("one_leaf")
    pop = device.PointPopulation(grid, 300)
    p = pop._ptr
    flags = t.ones(300, dtype=t.uint8, device="cuda")
    a, b = (t.full((300, 3), 7.0, device="cuda") for _ in range(2))
    field = t.full((512,), 1.0, device="cuda")
    vox = t.full((300,), 7, dtype=t.int32, device="cuda")
    SEL, COM, BIR, SIM = (f"hns_point_population_{k}" for k in ("select", "compact", "birth", "birth_sim"))
    _refused(lib.hns_point_population_compact(p, a.data_ptr(), b.data_ptr(), 12, None), COM, "no select")
    with pytest.raises(RuntimeError, match="no select"):
        pop.compact(a)
    _refused(lib.hns_point_population_select(p, flags.data_ptr(), 301, 1), SEL, "capacity")
    _refused(lib.hns_point_population_select(p, flags.data_ptr(), 2 ** 31, 1), SEL, "n is above")
    _refused(lib.hns_point_population_select(p, None, 300, 1), SEL, "d_flags")
    for bad in (0, 256, -1):
        _refused(lib.hns_point_population_select(p, flags.data_ptr(), 300, bad), SEL, "at_least")
    _refused(lib.hns_point_population_compact(p, a.data_ptr(), b.data_ptr(), 12, None), COM, "no select")  # (a refused select is no select)
    _refused(lib.hns_point_population_set_live(p, 2 ** 31), "hns_point_population_set_live", "n is above")
    info = _lib.hns_point_population_info()
    assert lib.hns_point_population_get(p, C.byref(info)) == 0 and (info.n, info.capacity) == (0, 300) and info.slot and info.counters
    _refused(lib.hns_point_population_get(p, None), "hns_point_population_get", "info")
    pop.select(flags[:257])
    for bad in (0, 2, 6, 68, -4):
        _refused(lib.hns_point_population_compact(p, a.data_ptr(), b.data_ptr(), bad, None), COM, "row_bytes")
    _refused(lib.hns_point_population_compact(p, a.data_ptr(), a.data_ptr(), 12, None), COM, "same buffer")
    _refused(lib.hns_point_population_compact(p, None, b.data_ptr(), 12, None), COM, "null")
    _refused(lib.hns_point_population_compact(p, a.data_ptr(), None, 12, None), COM, "null")

    def birth(field_ptr=field.data_ptr(), x=a.data_ptr(), v=vox.data_ptr(), rows=300, null_spec=False, **changes):
        s = leafio.birth_spec(**{**dict(threshold=0.25, rate=2.5, max_per_voxel=4, seed=1), **changes})
        return lib.hns_point_population_birth(p, field_ptr, None, None if null_spec else C.byref(s), x, v, rows, 0)

    _refused(birth(field_ptr=None), BIR, "d_field")
    _refused(birth(x=None), BIR, "d_xyz")
    _refused(birth(null_spec=True), BIR, "spec")
    _refused(birth(rows=2 ** 31), BIR, "capacity_rows")
    for k in (0, 17):
        _refused(birth(max_per_voxel=k), BIR, "max_per_voxel")
    for r in (0.0, -2.0, np.nan, np.inf):
        _refused(birth(rate=r), BIR, "rate")
    for th in (np.nan, -np.inf):
        _refused(birth(threshold=th), BIR, "threshold")
    _refused(birth(x=field.data_ptr()), BIR, "d_xyz is d_field")
    _refused(birth(x=vox.data_ptr()), BIR, "d_xyz is d_field or d_voxel")
    names = ["flame"]
    o = P.origins("one_leaf")
    _, sim = make_sim(o, names, random_state(1, 1, names), None, VS)  # a sim on a grid of its own over the same leaf
    spec = leafio.birth_spec(0.25, 2.5, 4, 1)
    _refused(lib.hns_point_population_birth_sim(p, sim._ptr, b"flame", 1, C.byref(spec), a.data_ptr(), vox.data_ptr(), 300, 0), SIM, "grid")
    with pytest.raises(ValueError, match="another grid"):
        sim.birth(pop, "flame", a, threshold=0.25, rate=2.5, max_per_voxel=4, seed=1)
    own = sim.point_population(10)
    _refused(lib.hns_point_population_birth_sim(own._ptr, sim._ptr, b"smoke", 1, C.byref(spec), a.data_ptr(), vox.data_ptr(), 300, 0), SIM, "smoke")
    _refused(lib.hns_point_population_birth_sim(own._ptr, sim._ptr, None, 1, C.byref(spec), a.data_ptr(), vox.data_ptr(), 300, 0), SIM, "field")
    _refused(lib.hns_point_population_birth_sim(own._ptr, None, b"flame", 1, C.byref(spec), a.data_ptr(), vox.data_ptr(), 300, 0), SIM, "null sim")
    with pytest.raises(ValueError, match="capacity"):
        pop.select(t.ones(301, dtype=t.uint8, device="cuda"))
    with pytest.raises(ValueError, match="row of src"):
        pop.compact(t.zeros((257, 17), device="cuda"))
    with pytest.raises(ValueError, match=r"\(rows, 3\)"):
        pop.birth(field, t.zeros((30, 4), device="cuda"), threshold=0.25, rate=2.5, max_per_voxel=4, seed=1)
    t.cuda.synchronize()
    assert bool((a == 7.0).all()) and bool((b == 7.0).all()) and bool((vox == 7).all()) and bool((field == 1.0).all()) and bool((flags == 1).all())
    assert pop.counts() == (257, 257) and own.counts() == (0, 0)  # (the refusals left the last select's count)
    err = C.c_int(0)
    assert lib.hns_point_population_create(P.host_grid("one_leaf").ptr, 16, C.byref(err)) is None
    _refused(err.value, "hns_point_population_create", "HNS_GRID_HOST_ONLY")
    new = sim.regrid(1)
    assert sim.grid is new
    with pytest.raises(RuntimeError, match="regrid"):
        own.select(flags[:10])
    own.close(), sim.close()
    pop.close()
    pop.close()
    for use in (lambda: pop.select(flags), lambda: pop.slot, lambda: pop.compact(a), lambda: pop.counts(), lambda: pop.set_live(1)):
        with pytest.raises(RuntimeError, match="closed"):
            use()
