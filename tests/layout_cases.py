"""TEST HELPER of tests/test_layout_cases.py (CPU) and tests/test_operand_layout_gpu.py: every entry point of include/hns.h that takes a device data pointer, run on
operands that are only as aligned as their element type.

include/hns.h ("Device operands") asks of a device pointer the alignment of its element type and promises that results do not depend on it. Everything else in the suite
hands the library tensors that torch allocated one by one (512-byte aligned) or views of a stream_cases.Slab at multiples of 256. Here EVERY operand of a call -- inputs
as well as outputs, and each pointer inside a `float* const*` list on its own -- is a view of one Slab that starts a few bytes behind a multiple of 256:

  "plus4"   every operand of 4-byte elements at +4, of 8-byte elements (int64 / uint64 counters, hns_stats records) at +8, every byte operand at +1
  "mixed"   the 4-byte-element operands of a call, in declaration order, at +12, +8, +4, +12, ...; 8-byte ones at +8; byte operands at +3, +2, +1, +3, ...
            The pointers of one call then differ mod 16: what exposes a kernel that tests one pointer and widens its access to another. +12 is `xyz[1:]` of an (n, 3) array.

The inputs are copied into their views before the call. Afterwards the guards are intact (the skipped bytes in front of a view are guard), the inputs outside `inplace`
are unchanged, and every output equals, byte for byte, (a) the same call on plain, separately allocated tensors and (b) the oracle or host mirror where the case has one.
No tolerance anywhere.

  LAYOUT_CASES   entry point -> Entry(level, source, grids, variants). Kernel level: the Call builders of stream_cases.py as they are, with their grids and their `expect`.
                 The calls without a stream parameter (the point order, the point population), which stream_cases cannot reach, and the sim-level point calls have builders
                 here, on the same Ctx data; at sim level only the caller-owned point arrays are operands (the fields belong to the library).
  LAYOUT_EXEMPT  entry point -> one of the four reasons below.
The coverage test in tests/test_layout_cases.py parses include/hns.h: a function with a data-pointer parameter that is in neither table, or in both, fails it. Neither
table may be extended from another module (see stream_cases.py on CASES / EXEMPT: a table that can grow elsewhere is no record of what was decided)."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

import stream_cases as sc
from stream_cases import MIRROR, N_POINTS, NS, ORACLE, SCATTERED, SIM_NAMES, Call, Entry, F, Slab, same_words, sentinel

LAYOUTS = ("plus4", "mixed")
STATS_OPERANDS = ("rec", "rec1", "rec3")  # hns_stats records travel as byte tensors (device.stats_buffer): their element is the 8-byte-aligned record


def element_bytes(name, dtype):
    return 8 if name in STATS_OPERANDS else np.dtype(dtype).itemsize


def skews(layout, operands):
    """operands: [(name, numpy dtype)] in declaration order -> {name: bytes behind a multiple of 256}. layout: one of LAYOUTS, or {name: bytes} as it is (a name left
    out: 0) for a test that places single operands"""
    if isinstance(layout, dict):
        return {name: int(layout.get(name, 0)) for name, _ in operands}
    assert layout in LAYOUTS, layout
    out, n4, n1 = {}, 0, 0
    for name, dtype in operands:
        e = element_bytes(name, dtype)
        assert e in (1, 4, 8), (name, dtype)
        if e == 8:
            out[name] = 8
        elif e == 4:
            out[name] = 4 if layout == "plus4" else (12, 8, 4)[n4 % 3]
            n4 += 1
        else:
            out[name] = 1 if layout == "plus4" else (3, 2, 1)[n1 % 3]
            n1 += 1
    return out


def operands_of(call):
    """[(name, dtype)] of a Call in declaration order: its inputs, then its outputs"""
    return [(k, v.dtype) for k, v in call.inputs.items()] + [(k, np.dtype(d)) for k, (_, d) in call.outputs.items()]


def specs_of(call):
    specs = {k: (v.shape, v.dtype) for k, v in call.inputs.items()}
    specs.update(call.outputs)
    return specs


def carve(torch, call, layout, device="cpu"):
    """the Slab of a call under a layout: every operand a view of it"""
    return Slab(torch, specs_of(call), device, skews(layout, operands_of(call)))


# ---------------------------------------------------------------------------------------------------------------------
# one run
# ---------------------------------------------------------------------------------------------------------------------


def _collect(torch, call, t, returned):
    torch.cuda.synchronize()
    got = {k: t[k].cpu().numpy().copy() for k in list(call.inplace) + list(call.outputs)}
    for k, v in (returned if isinstance(returned, dict) else {}).items():
        got[k] = v.cpu().numpy().copy() if torch.is_tensor(v) else np.array(v)
    return got


def run_plain(torch, call):
    """the call on separately allocated tensors -> {output: array}"""
    t = NS({k: torch.from_numpy(np.array(v)).cuda() for k, v in call.inputs.items()})
    for k, (shape, dtype) in call.outputs.items():
        t[k] = torch.empty(shape, dtype=sc._torch_dtype(torch, dtype), device="cuda")
        sentinel(t[k])
    torch.cuda.synchronize()
    return _collect(torch, call, t, call.run(t))


def run_skewed(torch, call, layout, what, run=None):
    """the call with every operand carved from one Slab under `layout` -> ({output: array}, the slab); guards and inputs are checked here"""
    slab = carve(torch, call, layout, "cuda")
    t = slab.views
    for k, v in call.inputs.items():
        t[k].copy_(torch.from_numpy(np.array(v)))
    for k in call.outputs:
        sentinel(t[k])
    torch.cuda.synchronize()
    got = _collect(torch, call, t, (run or call.run)(t))
    slab.check(what)
    sc.assert_inputs_unchanged({k: t[k] for k in call.inputs}, call.inputs, call.inplace, what)
    return got, slab


def assert_skewed(slab, call, layout):
    """the case cannot silently run aligned: every view starts where the layout says, and some float operand is off the 16-byte grid by 4, 8 or 12"""
    want = skews(layout, operands_of(call))
    for k, v in slab.views.items():
        assert v.data_ptr() % 256 == want[k], (k, v.data_ptr() % 256, want[k])
    floats = [v.data_ptr() % 16 for k, v in slab.views.items() if v.element_size() == 4]  # (float and 32-bit integer operands; hns_point_population_select has neither)
    assert (floats or set(slab.views) == {"flags"}) and (all(r == 4 for r in floats) if layout == "plus4" else floats[:1] in ([12], [])), floats


_SHARED = {}  # (entry point, variant, grid) -> (plain run's outputs, expected outputs or None): computed once, shared by both layouts, never written


def check_layout(torch, x, name, variant, layout):
    import hnanosolver_amd as H

    call = LAYOUT_CASES[name].variants[variant](x)
    what = f"{name}[{variant}] on {x.name}, layout {layout}"
    try:
        for k, v in call.options.items():
            H.set_option(k, v)
        key = (name, variant, x.name)
        if key not in _SHARED:
            _SHARED[key] = (run_plain(torch, call), call.expect(NS(call.inputs)) if call.expect is not None else None)
        plain, expected = _SHARED[key]
        got, slab = run_skewed(torch, call, layout, what)
        assert_skewed(slab, call, layout)
        sc.assert_same_outputs(got, plain, f"{what}, against the call on separately allocated tensors")
        for k, v in (expected or {}).items():
            assert same_words(got[k], v), f"{what}: output {k} differs from the oracle / host mirror"
            assert same_words(plain[k], v), f"{what}: output {k} of the plain run differs from the oracle / host mirror"
        return got
    finally:
        for k in call.options:
            H.set_option(k, None)


# ---------------------------------------------------------------------------------------------------------------------
# the calls without a stream parameter: the point order and the point population, on Ctx("scattered")'s points
# ---------------------------------------------------------------------------------------------------------------------


def _D():
    from hnanosolver_amd import device

    return device


class _closing:
    """a PointOrder / PointPopulation / Sim for one run: the device is idle when it goes back"""

    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        import torch

        torch.cuda.synchronize()
        self.obj.close()


def _order(x, t, level="voxel"):
    o = _D().PointOrder(x.grid, N_POINTS)
    o.sort(t.xyz, level)
    return _closing(o)


def o_sort(level):
    def build(x):
        import order_cases as oc

        def run(t):
            with _order(x, t, level) as o:
                return {"perm": o.perm.clone(), "keys": o.keys.clone(), "leaf_start": o.leaf_start.clone()}

        expect = lambda h: dict(zip(("perm", "keys", "leaf_start"), oc.restate(x.grid, x.nl, h.xyz, oc.LEVELS[("leaf", "voxel").index(level)])))
        return Call({"xyz": x.xyz}, {}, run, expect)
    return build


def _rows(seed, row_bytes):
    return np.random.default_rng(seed).standard_normal((N_POINTS, row_bytes // 4)).astype(F)


def o_move(which, row_bytes):
    def build(x):
        import order_cases as oc

        def run(t):
            with _order(x, t) as o:
                getattr(o, which)(t.src, t.dst)

        def expect(h):
            perm = oc.restate(x.grid, x.nl, h.xyz, 1)[0].astype(np.int64)
            dst = np.empty_like(h.src)
            if which == "gather":
                dst[:] = h.src[perm]
            else:
                dst[perm] = h.src
            return {"dst": dst}

        return Call({"xyz": x.xyz, "src": _rows(21, row_bytes)}, {"dst": ((N_POINTS, row_bytes // 4), F)}, run, expect)
    return build


def _splat_points(x):
    """Ctx's points behind binned_cases' two planted ones: a tail point and a binned point that reach one voxel"""
    import binned_cases as bc

    return np.ascontiguousarray(np.concatenate([bc.planted(x.origins), x.xyz[:-bc.N_PLANTED]]), dtype=F)


def o_splat(x):
    def run(t):
        with _order(x, t) as o:
            o.splat([t.density, t.vel], t.xyz, [t.vals, t.vals3], status=t.status, rejected=t.rejected)

    def expect(h):
        from hnanosolver_amd import api

        fields, status = [np.array(h.density), np.array(h.vel)], np.zeros(N_POINTS, np.uint8)
        rejected = api.splat_points_host(x.grid, fields, h.xyz, [h.vals, h.vals3], status=status)
        return {"density": fields[0], "vel": fields[1], "status": status, "rejected": np.array([rejected], dtype=np.int64)}

    ins = {"density": x.f["density"], "vel": x.f["vel"], "xyz": _splat_points(x), "vals": x.values, "vals3": x.values3, "rejected": np.zeros(1, np.int64)}
    return Call(ins, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("density", "vel", "rejected"))


NEIGHBOUR_RADIUS = 2.0


def _crowd(x):
    """1,000 points inside three leaves of the grid -- some twenty neighbours each at radius 2 -- in front of 31 of Ctx's scattered points (outside points and specials)"""
    rng = np.random.default_rng(61)
    inside = x.origins[rng.integers(0, 3, N_POINTS - 31)] + rng.uniform(0.0, 8.0, (N_POINTS - 31, 3))
    return np.ascontiguousarray(np.concatenate([inside.astype(F), x.xyz[-31:]]), dtype=F)


def o_neighbours(x):
    import neighbour_cases as nc

    def run(t):
        with _order(x, t) as o:
            o.neighbours(t.xyz, NEIGHBOUR_RADIUS, count=t.count, density=t.density, push=t.push)

    def expect(h):
        r = nc.restate(x.grid, x.nl, h.xyz, NEIGHBOUR_RADIUS)
        assert int((r.count >= 4).sum()) >= 900, "the case's points have too few neighbours"
        return {"count": r.count, "density": r.density, "push": r.push}

    return Call({"xyz": _crowd(x)}, {"count": ((N_POINTS,), np.int32), "density": ((N_POINTS,), F), "push": ((N_POINTS, 3), F)}, run, expect)


def _flags():
    return np.random.default_rng(31).integers(0, 3, N_POINTS).astype(np.uint8)


def p_select(x):
    import population_cases as pp

    def run(t):
        with _closing(_D().PointPopulation(x.grid, N_POINTS)) as p:
            p.select(t.flags, 1)
            return {"slot": p.slot.clone(), "counts": np.array(p.counts())}

    def expect(h):
        slot, live = pp.restate_select(h.flags, 1)
        return {"slot": slot, "counts": np.array([live, live])}

    return Call({"flags": _flags()}, {}, run, expect)


FILL_WORD = 0x7FC00000


def p_compact(row_bytes, fill):
    def build(x):
        import population_cases as pp

        def run(t):
            with _closing(_D().PointPopulation(x.grid, N_POINTS)) as p:
                p.select(t.flags, 1).compact(t.src, t.dst, FILL_WORD if fill else None)

        expect = lambda h: {"dst": pp.restate_compact(h.src, h.dst, h.flags, 1, FILL_WORD if fill else None)}
        return Call({"flags": _flags(), "src": _rows(22, row_bytes), "dst": _rows(23, row_bytes)}, {}, run, expect, inplace=("dst",))
    return build


BIRTH_ROWS = 4099
BIRTH_SPEC = dict(threshold=0.25, rate=2.5, max_per_voxel=4, seed=20)  # population_cases.SPEC


def _birth_field(x):
    """one voxel in 128 uniform in -0.5 .. 2, the rest 0: some 2,000 births, fewer than BIRTH_ROWS, so the fill has rows to write"""
    rng = np.random.default_rng(41)
    return np.where(rng.random(x.N) < 1.0 / 128.0, rng.uniform(-0.5, 2.0, x.N), 0.0).astype(F)


def p_birth(with_masks):
    def build(x):
        import population_cases as pp

        def run(t):
            with _closing(_D().PointPopulation(x.grid, BIRTH_ROWS)) as p:
                p.birth(t.field, t.xyz, masks=t.masks, voxel=t.voxel, **BIRTH_SPEC)
                return {"counts": np.array(p.counts())}

        def expect(h):
            xyz, voxel, live, wanted = pp.restate_birth(x.origins, h.field, h.masks, capacity_rows=BIRTH_ROWS, **BIRTH_SPEC)
            assert 100 <= wanted < BIRTH_ROWS
            return {"xyz": xyz, "voxel": voxel, "counts": np.array([live, wanted])}

        ins = {"field": _birth_field(x), **({"masks": x.masks} if with_masks else {})}
        return Call(ins, {"xyz": ((BIRTH_ROWS, 3), F), "voxel": ((BIRTH_ROWS,), np.int32)}, run, expect)
    return build


# ---------------------------------------------------------------------------------------------------------------------
# sim level: the fields are the library's; the caller-owned point arrays are the operands
# ---------------------------------------------------------------------------------------------------------------------


def _sim(x, masks=False):
    sim = _D().Sim(x.grid, SIM_NAMES)
    sim.upload(x.state)
    if masks:
        sim.set_active_masks(x.masks)
    return _closing(sim)


def _sim_state(sim):
    """the sim's fields, domain and masks on the idle device: {name: array}"""
    import torch
    from frame_cases import download

    torch.cuda.synchronize()
    out = {f"field {k}": v for k, v in download(sim, SIM_NAMES).items()}
    out["leaf origins"] = sim.grid.coords()[::512].copy()
    out["masks"] = sim.active_masks()
    return out


def _ok(rc):
    from hnanosolver_amd.api import _raise

    _raise(rc)


def _names(names):
    return (C.c_char_p * len(names))(*[k.encode() for k in names])


def _pointers(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def s_sample(x):
    D = _D()

    def run(t):
        with _sim(x) as sim:
            outs = [t[f"out_{k}"] for k in SIM_NAMES] + [t.out_vel]
            _ok(D.lib.hns_sim_sample_points(sim._ptr, _names(SIM_NAMES), len(SIM_NAMES), 1, D._ptr(t.xyz), N_POINTS, _pointers(outs), D.current_stream()))

    def expect(h):
        from points_cases import fma_branch

        out = {f"out_{k}": x.oracle.sample_trilinear_f(x.state[k], h.xyz) for k in SIM_NAMES}
        with fma_branch(x.oracle.L):
            out["out_vel"] = x.oracle.sample_trilinear_v(x.state["vel"], h.xyz)
        return out

    return Call({"xyz": x.xyz}, {**{f"out_{k}": ((N_POINTS,), F) for k in SIM_NAMES}, "out_vel": ((N_POINTS, 3), F)}, run, expect)


def s_trace(x):
    D = _D()

    def run(t):
        with _sim(x) as sim:
            _ok(D.lib.hns_sim_trace_points(sim._ptr, D._ptr(t.xyz), N_POINTS, x.dt, x.vs, 4, 3, D._byte_ptr(t.status), D.current_stream()))

    def expect(h):
        from points_cases import trace_mirror

        path, status = trace_mirror(x.oracle, x.state["vel"], h.xyz, x.dt, x.inv_dx, 4, 3)
        return {"xyz": path[-1], "status": status}

    return Call({"xyz": x.xyz}, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("xyz",))


def s_trace_collide(x):
    D = _D()

    def run(t):
        spec = D._collision("layout_cases", sc.COLLIDE_MODE, sc.COLLIDE_SPEC["threshold"], sc.COLLIDE_SPEC["skin"], sc.COLLIDE_SPEC["iterations"])
        with _sim(x) as sim:
            _ok(D.lib.hns_sim_trace_points_collide(sim._ptr, D._ptr(t.xyz), N_POINTS, x.dt, x.vs, sc.COLLIDE_ORDER, sc.COLLIDE_STEPS, C.byref(spec), D._byte_ptr(t.status),
                                                   D._byte_ptr(t.hit), D.current_stream()))

    def expect(h):
        got, status, hit = sc._collide_mirror(x, x.state["vel"], x.state["collision_sdf"], h.xyz)
        return {"xyz": got, "status": status, "hit": hit}

    return Call({"xyz": x.xyz}, {"status": ((N_POINTS,), np.uint8), "hit": ((N_POINTS,), np.uint8)}, run, expect, inplace=("xyz",))


def _sim_splat_call(x, through_order):
    D = _D()

    def run(t):
        with _sim(x, masks=True) as sim:
            args = (_names(["density", "fuel"]), 2, D._ptr(t.vals3), D._ptr(t.xyz), _pointers([t.vals, t.vals]))
            if through_order:
                with _closing(sim.point_order(N_POINTS)) as o:
                    o.sort(t.xyz)
                    _ok(D.lib.hns_point_order_splat_sim(o._live(), sim._ptr, *args, 0, -32, 1, D._byte_ptr(t.status), D._u64_ptr(t.rejected)))
            else:
                _ok(D.lib.hns_sim_splat_points(sim._ptr, *args, N_POINTS, -32, 1, D._byte_ptr(t.status), D._u64_ptr(t.rejected), D.current_stream()))
            return _sim_state(sim)

    def expect(h):
        from hnanosolver_amd import api

        fields, masks = [np.array(x.state["density"]), np.array(x.state["fuel"]), np.array(x.state["vel"])], np.array(x.masks)
        status = np.zeros(N_POINTS, np.uint8)
        rejected = api.splat_points_host(x.grid, fields, h.xyz, [h.vals, h.vals, h.vals3], masks=masks, status=status)
        return {"field density": fields[0], "field fuel": fields[1], "field vel": fields[2], "masks": masks, "status": status, "rejected": np.array([rejected], dtype=np.int64)}

    ins = {"xyz": _splat_points(x), "vals": x.values, "vals3": x.values3, "rejected": np.zeros(1, np.int64)}
    return Call(ins, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("rejected",))


def s_splat(x):
    return _sim_splat_call(x, False)


def o_splat_sim(x):
    return _sim_splat_call(x, True)


def p_birth_sim(x):
    import population_cases as pp

    field = x.state["density"]
    threshold = float(np.sort(field)[-(x.N // 128)])  # one voxel in 128 lies above it
    spec = dict(threshold=threshold, rate=float(F(2.5) / F(threshold)), max_per_voxel=4, seed=20)

    def run(t):
        with _sim(x, masks=True) as sim, _closing(sim.point_population(BIRTH_ROWS)) as p:
            sim.birth(p, "density", t.xyz, t.voxel, **spec)
            return {"counts": np.array(p.counts())}

    def expect(h):
        xyz, voxel, live, wanted = pp.restate_birth(x.origins, field, x.masks, capacity_rows=BIRTH_ROWS, **spec)
        assert 100 <= wanted, wanted
        return {"xyz": xyz, "voxel": voxel, "counts": np.array([live, wanted])}

    return Call({}, {"xyz": ((BIRTH_ROWS, 3), F), "voxel": ((BIRTH_ROWS,), np.int32)}, run, expect)


def s_regrid_seeded(x):
    def run(t):
        with _sim(x, masks=True) as sim:
            sim.regrid(1, points=t.xyz)
            return {"seeds skipped": np.array([sim.last_seeds_skipped]), **_sim_state(sim)}

    def expect(h):
        from seed_cases import host_chain_seeded

        dom, dm, out = host_chain_seeded(x.origins, x.masks, x.state, SIM_NAMES, 1, h.xyz)
        return {"leaf origins": dom, "masks": dm, **{f"field {k}": v for k, v in out.items()}}

    return Call({"xyz": x.xyz}, {}, run, expect)


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------

ROW_BYTES = (4, 12, 16, 64)
_ORDER = MIRROR + " (order_cases.restate)"
_POPULATION = MIRROR + " (population_cases)"

LAYOUT_CASES = {name: e for name, e in sc.CASES.items() if e.level == "kernel"}  # hns_dev_*: stream_cases' own builders, grids and expectations
LAYOUT_CASES.update({
    "hns_point_order_sort": Entry("order", _ORDER, SCATTERED, {"voxel": o_sort("voxel"), "leaf": o_sort("leaf")}),
    "hns_point_order_gather": Entry("order", _ORDER, SCATTERED, {f"rows_of_{b}": o_move("gather", b) for b in ROW_BYTES}),
    "hns_point_order_scatter": Entry("order", _ORDER, SCATTERED, {f"rows_of_{b}": o_move("scatter", b) for b in ROW_BYTES}),
    "hns_point_order_splat": Entry("order", MIRROR + " (hns_grid_splat_points; binned_cases.planted)", SCATTERED, {"float_and_vec3": o_splat}),
    "hns_point_order_neighbours": Entry("order", MIRROR + " (neighbour_cases.restate)", SCATTERED, {"radius_2": o_neighbours}),
    "hns_point_population_select": Entry("population", _POPULATION, SCATTERED, {"at_least_1": p_select}),
    "hns_point_population_compact": Entry("population", _POPULATION, SCATTERED, {f"rows_of_{b}{'_fill' if f else ''}": p_compact(b, f) for b in ROW_BYTES for f in (False, True)}),
    "hns_point_population_birth": Entry("population", _POPULATION, SCATTERED, {"masked": p_birth(True), "all_voxels": p_birth(False)}),
    "hns_sim_sample_points": Entry("sim", ORACLE + " (sample_trilinear_f / _v)", SCATTERED, {"all_fields_and_velocity": s_sample}),
    "hns_sim_trace_points": Entry("sim", MIRROR + " (points_cases.trace_mirror)", SCATTERED, {"order4_steps3": s_trace}),
    "hns_sim_trace_points_collide": Entry("sim", MIRROR + " (points_collide_cases.collide_mirror)", SCATTERED, {sc.COLLIDE_VARIANT: s_trace_collide}),
    "hns_sim_splat_points": Entry("sim", MIRROR + " (hns_grid_splat_points)", SCATTERED, {"two_floats_and_velocity": s_splat}),
    "hns_point_order_splat_sim": Entry("sim", MIRROR + " (hns_grid_splat_points; binned_cases.planted)", SCATTERED, {"two_floats_and_velocity": o_splat_sim}),
    "hns_point_population_birth_sim": Entry("sim", _POPULATION, SCATTERED, {"density_masked": p_birth_sim}),
    "hns_sim_regrid_seeded": Entry("sim", MIRROR + " (seed_cases.host_chain_seeded)", SCATTERED, {"seeds_only": s_regrid_seeded}),
})

HOST = "host memory only: the arrays are the caller's host arrays; hipMemcpy or plain C++ reads them"
DIST = "hns_dist_*: the fields belong to the library; the caller's arrays are host memory"
TIMING = "timing helper around hns_dev_rbgs_iterate, which is a case; it returns no field"
OPERATOR = "operator path: host pointers, the library owns the device side"

LAYOUT_EXEMPT = {
    **{n: HOST for n in (
        "hns_grid_create", "hns_grid_create_from_leaves", "hns_grid_offsets", "hns_grid_neighbor_table", "hns_grid_coords", "hns_grid_matches", "hns_grid_export_nanovdb",
        "hns_grid_launch_tables", "hns_gather_leaves", "hns_scatter_leaves", "hns_dilate_leaves", "hns_dilate_leaf_masks", "hns_union_leaves", "hns_add_leaves",
        "hns_deactivate_leaf_masks", "hns_leaf_stats", "hns_grid_splat_points", "hns_grid_splat_points_spec", "hns_point_leaves", "hns_grid_sort_points",
        "hns_grid_point_neighbours", "hns_grid_birth_points", "hns_sim_set_active_masks", "hns_sim_active_masks", "hns_sim_regrid", "hns_sim_regrid_sourced",
        "hns_sim_stats", "hns_sim_residual", "hns_sim_solve_report", "hns_sim_pressure_time", "hns_sim_stage_times", "hns_sim_regrid_times")},
    **{n: DIST for n in (
        "hns_dist_create", "hns_dist_unique_id", "hns_dist_connect_rccl", "hns_dist_ipc_export", "hns_dist_connect_ipc", "hns_dist_peer_region", "hns_dist_upload",
        "hns_dist_download", "hns_dist_download_local", "hns_dist_pressure_time")},
    "hns_dev_time_rbgs": TIMING,
    "hns_compute_sim_resident": OPERATOR,
}
REASONS = (HOST, DIST, TIMING, OPERATOR)


def variants(levels=None):
    """[(entry point, variant id, grid name)] for pytest.mark.parametrize"""
    return [(name, v, g) for name, e in LAYOUT_CASES.items() if levels is None or e.level in levels for v in e.variants for g in e.grids]


DATA_POINTER = re.compile(r"\b(?:const\s+)?(?:float|uint32_t|int32_t|unsigned\s+char|void|hns_stats)\s*\*(?:\s*const\s*\*)?\s*(\w+)?")
NO_DATA = ("stream", "hip_stream")  # void* parameters that are handles


def data_pointer_entry_points(header_text):
    """the functions include/hns.h declares with a parameter that points at data: float*, float* const*, uint32_t*, int32_t*, unsigned char*, void* rows and hns_stats*.
    Handles (hns_grid*, hns_sim*, ..., `void* stream`), `char*` text, `int*` / `uint64_t*` results and struct specs are not data pointers."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(hns_\w+)\s*\(([^;{}()]*?)\)\s*;", text, flags=re.S):
        for p in m.group(2).split(","):
            q = DATA_POINTER.search(p)
            if q and q.group(1) not in NO_DATA and "**" not in p.replace(" ", ""):
                out.append(m.group(1))
                break
    return out


# ---------------------------------------------------------------------------------------------------------------------
# aliasing: what include/hns.h permits and what it forbids, by the sentences in front of the prototypes
# ---------------------------------------------------------------------------------------------------------------------

MAY_ALIAS = ("hns_dev_subtract_pressure_gradient", "hns_dev_temperature_buoyancy")  # run in place by tests/test_operand_layout_gpu.py
MUST_NOT_ALIAS = ("hns_dev_advect_vector", "hns_dev_advect_scalars_ahead", "hns_dev_rbgs_iterate", "hns_dev_vorticity_confinement")  # called with overlapping buffers there


def alias_sentences(header_text, pattern):
    """the functions whose comment (the one in front of the prototype) says `pattern`; the header's opening comment, which states the rule, is no function's"""
    out = set()
    for m in re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*[\w\s\*]*?\b(hns_\w+)\s*\(", header_text, flags=re.S):
        if re.search(pattern, m.group(1)):
            out.add(m.group(2))
    return out
