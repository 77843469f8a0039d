"""TEST HELPER of tests/test_sequence_cases.py (CPU) and tests/test_sequences_gpu.py: mixed call sequences on ONE device-resident sim against a twin with no hidden state.

A sim and the point objects that hang off it carry state between calls. Some of it is semantic -- include/hns.h documents it as the sim's or the object's state -- and
the rest is memo: the look-ahead, the feedback signatures, `solved` and p_result, the multigrid hierarchy, the lazily made tables, the buffer roles that swap under
every call, the grid's pooled splat accumulator, an order's permutation and its cell table, and a population's slots. A stale memo gives plausible numbers and no fault.

  OPS       the vocabulary: one entry per call that changes or reads that state, a function (world, rng) -> outputs with the resources it reads and writes, the
            library symbols it goes through, what it needs from the script before it, and what it does to the look-ahead memo.
  World     the device side of a script: the sim, the points, one PointOrder and one PointPopulation, and one PointMotion of N_POINTS rows, one Shaping and one Diffusion.
  resident  ONE World from the first step to the last (the order and the population made anew only after a step that moves the sim onto another grid; the motion, the
            shaping and the diffusion are bound to no grid and stay through every change of grid: the Diffusion with its pooled block, the motion with its rows).
  twin      a NEW World for every step, built from nothing but the semantic state (`World.capture`), run with lookahead = 0 and the pool filled with a non-zero byte.
  SCRIPTS   the committed scripts: explicit lists of (operation, seed). `draw_scripts` is the seeded generator the first twelve were drawn with, the rest are written by
            hand (POINT_SCRIPTS: collision tracing, the order's cell table, the frame loop of points) or drawn by `draw_scripts(only=...)` for the pairs a grown table
            adds (FEATURE_SCRIPTS: points with a velocity of their own, shaping, diffusion); a red script is rerun and cut down by hand with `compare(script, mode, upto=...)`.

Every comparison is equality of bytes: every path involved is documented as bit-identical to its stateless form. Where a memo may rightly live or die without moving a
byte -- hns_sim_deactivate drops the look-ahead although the velocity stays; a decay or a diffuse of float fields alone must keep it -- the table's memo column predicts hns_sim_lookahead_counts under lookahead = 1
(`expected_lookahead`), and the resident pass is held to it step by step. Everything runs on the null stream."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import frame_cases as fc

F = np.float32
DT = float(F(1.0 / 24.0))  # of every substep, advect and trace of every script: "two substeps of equal dt and voxel size" is then any two substeps
VS = 1.0 / 32
ITERS = 3
N_POINTS = 1500
TWIN_FILLS = (0x7F, 0xFF)  # the pool's fill byte during the twin's pass, by the parity of the step: a finite 3.39e38 and a NaN
PROFILES = {"combust": list(fc.COMBUST), "collide": list(fc.COMBUST) + ["collision_sdf"], "one": ["density"]}

# ---- resources ---------------------------------------------------------------------------------------------------------------------------------------------------

ALL_FIELDS = tuple("f:" + n for n in PROFILES["collide"])
ADVECTED = tuple("f:" + n for n in fc.COMBUST)
RESOURCES = ("vel", "masks", "grid", "scratch", "splat_spec", "solve_method", "solve_control", "points", "order", "cells", "live", "motion") + ALL_FIELDS
# cells: the order's cell table, a memo of "order"; motion: rows 0 .. N_POINTS - 1 of the PointMotion's xyz, vel and age (status and hit are outputs of a step)
SOLVE = ("solve_method", "solve_control", "grid")  # what every pressure solve reads besides its right-hand side (the hierarchy is a memo of grid and method)


class Op(NamedTuple):
    kind: str
    fn: object
    reads: frozenset
    writes: frozenset
    symbols: tuple
    needs: frozenset     # float fields the sim must hold
    requires: frozenset  # "order": a sort since the last change of grid; "fresh_order": and no write of the positions since; "voxel_order": and the last sort by voxel
    grid: bool           # moves the sim onto another grid
    memo: str            # what the call does to the look-ahead memo under lookahead = 1: "produce" (consumes a live one, leaves one), "consume" (consumes a live one,
                         # leaves none), "drop", or "keep"
    same_points: bool    # writes the point arrays with the bytes they held (scatter of gather)
    sets: frozenset      # what the call establishes of `requires` for the steps behind it (the sorts)
    clears: frozenset    # ... and what it takes away besides what `breaks` works out (a sort by leaf: "voxel_order")

    @property
    def breaks(self):
        out = set(self.clears)
        if self.grid:
            out |= {"order", "fresh_order", "voxel_order"}
        if "points" in self.writes and not self.same_points:
            out.add("fresh_order")
        return frozenset(out)


OPS = {}


def op(kind, reads=(), writes=(), symbols=(), needs=(), requires=(), grid=False, memo="keep", same_points=False, sets=(), clears=()):
    def add(fn):
        w = set(writes) | ({"grid", "scratch"} if grid else set())
        OPS[fn.__name__] = Op(kind, fn, frozenset(reads), frozenset(w), tuple(symbols), frozenset(needs), frozenset(requires), grid, memo, same_points, frozenset(sets),
                              frozenset(clears))
        return fn

    return add


# the symbols the two runners and World go through themselves, whatever the script
RUNNER_SYMBOLS = ("hns_sim_create", "hns_sim_destroy", "hns_sim_upload", "hns_sim_download", "hns_sim_set_active_masks", "hns_sim_active_masks", "hns_sim_get_splat_spec",
                  "hns_sim_set_splat_spec", "hns_sim_set_solve_method", "hns_sim_set_solve_control", "hns_sim_lookahead_counts", "hns_sim_timing", "hns_sim_pressure_time",
                  "hns_sim_stage_timing", "hns_sim_stage_times", "hns_point_order_create", "hns_point_order_destroy", "hns_point_order_set_stream", "hns_point_order_get",
                  "hns_point_order_sort", "hns_point_population_create", "hns_point_population_destroy", "hns_point_population_set_stream", "hns_point_population_set_live",
                  "hns_point_population_get", "hns_point_population_counts", "hns_point_motion_create", "hns_point_motion_destroy", "hns_point_motion_set_stream",
                  "hns_point_motion_get", "hns_shaping_create", "hns_shaping_destroy", "hns_shaping_set_stream", "hns_diffusion_create", "hns_diffusion_destroy",
                  "hns_diffusion_set_stream")

EXEMPT = {
    "hns_sim_velocity_ptr": "switches the look-ahead off for good by contract, so no memo is left to go stale behind it; test_lookahead_gpu holds that contract",
    "hns_sim_substep_plan": "its text names the memo by design (advect_vector=memo), so a resident sim and a twin differ in it rightly; test_kernel_variants_gpu reads it",
    "hns_point_order_splat": "writes caller-owned tensors and no sim buffer: there is no sim state for it to leave stale; the sim's form hns_point_order_splat_sim is an operation",
    "hns_point_population_birth": "reads a caller-owned tensor and no sim: the sim's form hns_point_population_birth_sim is an operation and shares its kernels",
    "hns_shaping_curl_host": "host-only: it evaluates one voxel's curl from a host struct and touches no sim, no object and no device; test_shaping_cases holds it to the mirror",
    "hns_diffusion_schedule_host": "host-only: it forms one coefficient's constants from numbers and touches no sim, no object and no device; test_diffusion_cases holds it",
}


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------------------


def _torch():
    import torch

    return torch


def device_floats(owner, ptr, n):
    """`n` floats of device memory at `ptr` as a torch view (no copy)"""
    from hnanosolver_amd import device

    torch = _torch()
    return torch.as_tensor(device._DeviceWords(ptr, n, owner), device="cuda").view(torch.float32)


DEFAULT_SPEC = (0, 0, 0.0, 0.0)
MOTION_STATE = ("xyz", "vel", "age")  # the PointMotion's arrays that are state; the state's keys are "motion_xyz", ...


class World:
    """The sim of a script with its points, its order, its population, its motion, its shaping and its diffusion, opened from the semantic state alone: what `capture`
    returns (the motion's xyz, vel and age with it; its status and hit are outputs of a step and hold pool contents before the first), plus the solve method, the solve
    control, the order's last (xyz, level) and the switches of the script, which the library has no getter for and the ops record here."""

    def __init__(self, state):
        from hnanosolver_amd import api, device

        torch = _torch()
        self.names = list(state["names"])
        self.timing = state["timing"]
        self.grid = api.create_grid_from_leaves(state["origins"], VS)
        self.grids = [self.grid]  # every grid the sim has been on: none is freed mid-script
        self.sim = device.Sim(self.grid, self.names)
        self.sim.upload({k: np.ascontiguousarray(state[k]) for k in ["vel"] + self.names})
        if state["masks"] is not None:
            self.sim.set_active_masks(state["masks"])
        self.set_spec(state["splat_spec"])
        self.method = self.control = None
        self.set_method(state["method"])
        self.set_control(state["control"])
        if self.timing:
            self.sim.timing(64)
            self.sim.stage_timing(64)
        self.xyz = torch.from_numpy(np.array(state["xyz"])).cuda()
        self.attr = torch.from_numpy(np.array(state["attr"])).cuda()
        self.order_key = state["order_key"]
        self.live = state["live"]
        self._order = self._population = None
        # bound to no grid (include/hns.h): these three stay from the first step to the last, through every change of grid -- `after` does not drop them
        self.motion = device.PointMotion(N_POINTS)
        self.shaping, self.diffusion = device.Shaping(), device.Diffusion()
        for k in MOTION_STATE:
            getattr(self.motion, k).copy_(torch.from_numpy(np.array(state["motion_" + k])).cuda())

    # -- the state the library has no getter for
    def set_spec(self, spec):
        from hnanosolver_amd import _lib, api

        kernel, mode, radius, min_weight = spec
        api._raise(_lib.lib.hns_sim_set_splat_spec(self.sim._ptr, C.byref(_lib.hns_splat_spec(kernel, mode, radius, None, min_weight))))

    def get_spec(self):
        from hnanosolver_amd import _lib, api

        s = _lib.hns_splat_spec()
        api._raise(_lib.lib.hns_sim_get_splat_spec(self.sim._ptr, C.byref(s)))
        assert not s.d_radius
        return (int(s.kernel), int(s.mode), float(s.radius), float(s.min_weight))

    def set_method(self, method):
        self.method = method
        self.sim.solve_method(None) if method is None else self.sim.solve_method(1, *method)

    def set_control(self, control):
        self.control = control
        self.sim.solve_control(None) if control is None else self.sim.solve_control(*control)

    # -- the point objects
    def order(self):
        """the PointOrder on the sim's current grid; a new one sorts the order's last (xyz, level) again"""
        if self._order is None:
            self._order = self.sim.point_order(N_POINTS)
            if self.order_key is not None:
                self._order.sort(_torch().from_numpy(self.order_key[0]).cuda(), self.order_key[1])
        return self._order

    def population(self):
        """the PointPopulation on the sim's current grid; a new one is told the live count"""
        if self._population is None:
            self._population = self.sim.point_population(N_POINTS)
            if self.live is not None:
                self._population.set_live(self.live)
        return self._population

    def drop_point_objects(self):
        for o in (self._order, self._population):
            if o is not None:
                o.close()
        self._order = self._population = None

    def after(self, operation: Op):
        if operation.grid:  # the objects of the old grid refuse every call from here on
            self.grids.append(self.sim.grid)
            self.drop_point_objects()
            self.order_key = None

    def vel3(self):
        """an (n, 3) value per point from the attribute"""
        a = self.attr
        return _torch().stack([a, -0.5 * a, 0.25 * a], dim=1).contiguous()

    def capture(self):
        """the full downloaded state: everything include/hns.h documents as the sim's and the objects' state, and nothing else"""
        sim = self.sim
        st = fc.download(sim, self.names)
        st.update(origins=np.ascontiguousarray(sim.grid.coords()[::512]), masks=sim.active_masks(), xyz=self.xyz.cpu().numpy(), attr=self.attr.cpu().numpy(),
                  splat_spec=self.get_spec(), live=self.live)
        st.update({"motion_" + k: getattr(self.motion, k).cpu().numpy() for k in MOTION_STATE})
        return st

    def carry(self, captured):
        """the state a new World is opened from"""
        return dict(captured, names=self.names, timing=self.timing, method=self.method, control=self.control, order_key=self.order_key)

    def close(self):
        if self.timing:  # (times are never compared)
            self.sim.pressure_time(), self.sim.stage_times()
        self.drop_point_objects()
        for o in (self.motion, self.shaping, self.diffusion):
            o.close()
        self.sim.close()


# ---- the vocabulary ----------------------------------------------------------------------------------------------------------------------------------------------


def _seed(rng):
    return int(rng.integers(1 << 30))


def _solve_outputs(w):
    """what a pressure solve leaves behind it for the host: the control's report and history, the hierarchy's levels"""
    out = {}
    if w.control is not None:
        r = w.sim.solve_report()
        out["solve_report"] = (r["iterations"], r["checks"], r["converged"], r["initial"].tobytes(), r["final"].tobytes())
        out["solve_history"] = r["history"]
    if w.method is not None:
        out["solve_levels"] = np.array(w.sim.solve_levels(), dtype=np.int64)
    return out


def _vel(rng, n):
    return fc.with_negative_zeros(rng, (0.6 * rng.standard_normal((n, 3))).astype(F))


@op("upload", writes=("vel",), symbols=("hns_sim_upload",), memo="drop")
def upload_vel(w, rng):
    w.sim.upload({"vel": _vel(rng, w.sim.grid.voxel_count())})
    return {}


@op("upload", writes=("f:density",), symbols=("hns_sim_upload",), memo="drop")
def upload_field(w, rng):
    w.sim.upload({"density": rng.standard_normal(w.sim.grid.voxel_count()).astype(F)})
    return {}


@op("upload", writes=("vel",) + ALL_FIELDS, symbols=("hns_sim_upload",), memo="drop")
def upload_all(w, rng):
    n = w.sim.grid.voxel_count()
    st = {"vel": _vel(rng, n)}
    for k in w.names:
        st[k] = fc.with_negative_zeros(rng, rng.standard_normal(n).astype(F))
    w.sim.upload(st)
    return {}


@op("core_substep", reads=("vel",) + ADVECTED + SOLVE, writes=("vel", "scratch") + ADVECTED, symbols=("hns_sim_core_substep",), memo="produce")
def core_substep(w, rng):
    w.sim.core_substep(ITERS, DT, VS)
    return _solve_outputs(w)


def _substep(w, params, collision, fuse=None):
    import hnanosolver_amd as H

    if fuse is not None:
        H.set_option("fuse", fuse)
    try:
        w.sim.substep(ITERS, DT, VS, params, collision)
    finally:
        H.set_option("fuse", None)
    return _solve_outputs(w)


@op("substep", reads=("vel",) + ADVECTED + SOLVE, writes=("vel", "scratch") + ADVECTED, symbols=("hns_sim_substep",), needs=fc.COMBUST, memo="consume")
def substep_fused(w, rng):
    from hnanosolver_amd import api

    return _substep(w, api.CombustionParams(), False)


@op("substep", reads=("vel",) + ADVECTED + SOLVE, writes=("vel", "scratch") + ADVECTED, symbols=("hns_sim_substep",), needs=fc.COMBUST, memo="produce")
def substep_unfused(w, rng):
    from hnanosolver_amd import api

    return _substep(w, api.CombustionParams(), False, fuse="0")


@op("substep", reads=("vel",) + ADVECTED + SOLVE, writes=("vel", "scratch") + ADVECTED, symbols=("hns_sim_substep",), needs=fc.COMBUST, memo="consume")
def substep_vorticity(w, rng):
    from hnanosolver_amd import api

    return _substep(w, api.CombustionParams(factorScale=1.0, vorticityScale=0.4), False)


@op("substep", reads=("vel",) + ALL_FIELDS + SOLVE, writes=("vel", "scratch") + ADVECTED, symbols=("hns_sim_substep",), needs=PROFILES["collide"], memo="drop")
def substep_collision(w, rng):
    from hnanosolver_amd import api

    return _substep(w, api.CombustionParams(), True)


@op("advect", reads=("vel", "f:density", "grid"), writes=("f:density",), symbols=("hns_sim_advect",), memo="drop")
def advect_names(w, rng):
    w.sim.advect(["density"], velocity=False, dt=DT, voxel_size=VS)
    return {}


@op("advect", reads=("vel", "grid") + ADVECTED, writes=("vel",) + ADVECTED, symbols=("hns_sim_advect",), memo="drop")
def advect_velocity(w, rng):
    w.sim.advect(None, velocity=True, dt=DT, voxel_size=VS)
    return {}


@op("pressure", reads=SOLVE, writes=("scratch",), symbols=("hns_sim_divergence_ptr", "hns_sim_pressure_solve", "hns_sim_residual", "hns_sim_pressure_ptr", "hns_sim_solve_report",
                                                           "hns_sim_solve_levels"))
def pressure_residual(w, rng):
    """ONE compound step, because div and p are scratch (include/hns.h): write div, solve, take the residual of that solve, read p"""
    from hnanosolver_amd._lib import lib

    n = w.sim.grid.voxel_count()
    div = device_floats(w.sim, lib.hns_sim_divergence_ptr(w.sim._ptr), n)
    div.copy_(_torch().from_numpy(rng.standard_normal(n).astype(F)))
    w.sim.pressure_solve(ITERS, VS)
    out = {"residual": w.sim.residual(VS)}
    out["p"] = device_floats(w.sim, lib.hns_sim_pressure_ptr(w.sim._ptr), n).clone().cpu().numpy()
    out.update(_solve_outputs(w))
    return out


def sparse_masks(rng, moving):
    """masks that shrink the next regrid's domain without emptying the sim: of the voxels that hold a velocity (`moving`, (leaves, 512) bool) a share per leaf, a third
    of those leaves none, and a dozen voxels anywhere"""
    n = len(moving)
    bits = moving & (rng.random((n, 512)) < rng.choice([0.05, 0.5, 1.0], size=(n, 1)))
    bits[rng.permutation(n)[: n // 3]] = False
    bits[rng.integers(n, size=12), rng.integers(512, size=12)] = True
    return fc.pack(bits)


@op("set_active_masks", reads=("grid",), writes=("masks",), symbols=("hns_sim_set_active_masks",))
def masks_array(w, rng):
    """(the harness looks at the downloaded velocity to choose the masks; the call itself reads no field)"""
    n = w.sim.grid.voxel_count()
    vel = np.empty((n, 3), dtype=F)
    w.sim.download({"vel": vel})
    w.sim.set_active_masks(sparse_masks(rng, (vel != 0).any(1).reshape(-1, 512)))
    return {}


@op("set_active_masks", writes=("masks",), symbols=("hns_sim_set_active_masks",))
def masks_none(w, rng):
    w.sim.set_active_masks(None)
    return {}


def _regrid(w, padding, **kw):
    before = w.sim.grid.leaf_count()
    w.sim.regrid(padding, **kw)
    if w.timing:
        w.sim.regrid_times()
    out = {"leaves": (before, w.sim.grid.leaf_count())}
    if w.method is not None:
        out["solve_levels"] = np.array(w.sim.solve_levels(), dtype=np.int64)
    return out


CARRIED = ("vel", "masks", "grid", "solve_method") + ALL_FIELDS  # what a regrid reads: everything it carries, and the method whose hierarchy it drops


@op("regrid", reads=CARRIED, writes=("vel", "masks") + ALL_FIELDS, symbols=("hns_sim_regrid", "hns_sim_regrid_times", "hns_sim_solve_levels"), grid=True, memo="drop")
def regrid_plain(w, rng):
    return _regrid(w, 1)


@op("regrid", reads=CARRIED, writes=("vel", "masks") + ALL_FIELDS, symbols=("hns_sim_regrid_sourced",), grid=True, memo="drop")
def regrid_sourced(w, rng):
    src = fc.make_sources(_seed(rng), w.sim.grid.coords()[::512], "mixed", "edge")
    return _regrid(w, 2, sources={k: v for k, v in src.items() if k == "vel" or k in w.names})


@op("regrid", reads=CARRIED + ("points",), writes=("vel", "masks") + ALL_FIELDS, symbols=("hns_sim_regrid_seeded",), grid=True, memo="drop")
def regrid_seeded(w, rng):
    out = _regrid(w, 0, points=w.xyz)
    out["seeds_skipped"] = w.sim.last_seeds_skipped
    return out


@op("regrid", reads=CARRIED, writes=("vel", "masks") + ALL_FIELDS, symbols=("hns_sim_regrid",), needs=("collision_sdf",), grid=True, memo="drop")
def regrid_sdf(w, rng):
    return _regrid(w, 1, sdf=fc.sdf_source(_seed(rng), w.sim.grid.coords()[::512]))


def _emit(w, **kw):
    before = w.sim.grid.leaf_count()
    rejected = _torch().zeros(1, dtype=_torch().int64, device="cuda")
    _, status = w.sim.emit({"density": w.attr}, w.xyz, rejected=rejected, **kw)
    return {"leaves": (before, w.sim.grid.leaf_count()), "status": status.cpu().numpy(), "rejected": int(rejected.item()), "seeds_skipped": w.sim.last_seeds_skipped}


EMIT_SYMBOLS = ("hns_sim_regrid_seeded", "hns_sim_splat_points")


@op("emit", reads=CARRIED + ("points",), writes=("vel", "masks") + ALL_FIELDS, symbols=EMIT_SYMBOLS, grid=True, memo="drop")
def emit_trilinear(w, rng):
    return _emit(w, padding=1)


@op("emit", reads=CARRIED + ("points",), writes=("vel", "masks") + ALL_FIELDS, symbols=EMIT_SYMBOLS, grid=True, memo="drop")
def emit_radial(w, rng):
    return _emit(w, velocity=w.vel3(), padding=2, radius=1.5)


QUIET = dict(tolerances={"density": 0.7}, velocity=1.0)


@op("deactivate", reads=("vel", "f:density", "masks", "grid"), writes=("masks",), symbols=("hns_sim_deactivate",), memo="drop")
def deactivate(w, rng):
    w.sim.deactivate(**QUIET)
    return {}


@op("deactivate", reads=("vel", "f:density", "masks", "grid"), writes=("masks",), symbols=("hns_sim_deactivate",), memo="drop")
def deactivate_counts(w, rng):
    return {"counts": w.sim.deactivate(counts=True, **QUIET)}


@op("stats", reads=("vel", "masks", "grid") + ALL_FIELDS, symbols=("hns_sim_stats",))
def stats(w, rng):
    return {"records": w.sim.stats(w.names, velocity=True, masks=True)}


@op("sample", reads=("vel", "grid", "points") + ALL_FIELDS, symbols=("hns_sim_sample_points", "hns_sim_field_ptr"))
def sample(w, rng):
    from hnanosolver_amd._lib import lib

    out = {k: v.cpu().numpy() for k, v in w.sim.sample(None, w.xyz, velocity=True).items()}
    out["density_in_place"] = device_floats(w.sim, lib.hns_sim_field_ptr(w.sim._ptr, b"density"), w.sim.grid.voxel_count()).cpu().numpy()
    return out


@op("trace", reads=("vel", "grid", "points"), writes=("points",), symbols=("hns_sim_trace_points",))
def trace(w, rng):
    return {"status": w.sim.trace(w.xyz, dt=DT, voxel_size=VS, order=2, steps=2, status=True).cpu().numpy()}


def _splat(w, values, velocity, **kw):
    rejected = _torch().zeros(1, dtype=_torch().int64, device="cuda")
    status = w.sim.splat(values, w.xyz, velocity, status=True, rejected=rejected, **kw)
    return {"status": status.cpu().numpy(), "rejected": int(rejected.item())}


SPLAT = ("hns_sim_splat_points",)


@op("splat", reads=("f:density", "masks", "grid", "points"), writes=("f:density", "masks"), symbols=SPLAT)
def splat_floats(w, rng):
    return _splat(w, {"density": w.attr}, None, activate=True)


@op("splat", reads=("vel", "grid", "points"), writes=("vel",), symbols=SPLAT, memo="drop")
def splat_velocity(w, rng):
    return _splat(w, {}, w.vel3(), activate=False)


@op("splat", reads=("vel", "f:density", "masks", "grid", "points"), writes=("vel", "f:density", "masks"), symbols=SPLAT, memo="drop")
def splat_both(w, rng):
    return _splat(w, {"density": w.attr}, w.vel3(), activate=True, kernel="radial", radius=1.25)


@op("splat", reads=("vel", "f:density", "masks", "grid", "points", "splat_spec"), writes=("vel", "f:density", "masks"), symbols=SPLAT, memo="drop")
def splat_stored(w, rng):
    """through the spec stored with the sim: the library call itself, which reads it (Sim.splat stores its keywords' spec for the call)"""
    from hnanosolver_amd import api
    from hnanosolver_amd._lib import lib

    torch = _torch()
    n = w.xyz.shape[0]
    status, rejected, vel = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), w.vel3()
    api._raise(lib.hns_sim_splat_points(w.sim._ptr, (C.c_char_p * 1)(b"density"), 1, vel.data_ptr(), w.xyz.data_ptr(), (C.c_void_p * 1)(w.attr.data_ptr()), n, -32, 1,
                                        status.data_ptr(), rejected.data_ptr(), 0))
    return {"status": status.cpu().numpy(), "rejected": int(rejected.item())}


def _sort(w, level):
    o = w.order()
    o.sort(w.xyz, level)
    w.order_key = (w.xyz.cpu().numpy(), level)
    return {"perm": o.perm.cpu().numpy(), "keys": o.keys.cpu().numpy(), "leaf_start": o.leaf_start.cpu().numpy()}


@op("sort", reads=("grid", "points"), writes=("order", "cells"), symbols=("hns_point_order_sort", "hns_point_order_get"), sets=("order", "fresh_order", "voxel_order"))
def sort_voxel(w, rng):
    return _sort(w, "voxel")


@op("sort", reads=("grid", "points"), writes=("order", "cells"), symbols=("hns_point_order_sort", "hns_point_order_get"), sets=("order", "fresh_order"), clears=("voxel_order",))
def sort_leaf(w, rng):
    return _sort(w, "leaf")


@op("gather_scatter", reads=("order", "points"), writes=("points",), symbols=("hns_point_order_gather", "hns_point_order_scatter"), requires=("order",), same_points=True)
def gather_scatter(w, rng):
    o = w.order()
    gx, ga = o.gather(w.xyz), o.gather(w.attr)
    w.xyz, w.attr = o.scatter(gx), o.scatter(ga)
    return {"ranked_xyz": gx.cpu().numpy(), "ranked_attr": ga.cpu().numpy()}


ORDER_SPLAT = ("hns_point_order_splat_sim",)


@op("order_splat", reads=("vel", "f:density", "masks", "grid", "points", "order"), writes=("vel", "f:density", "masks"), symbols=ORDER_SPLAT, requires=("order", "fresh_order"),
    memo="drop")
def order_splat_original(w, rng):
    return _splat(w, {"density": w.attr}, w.vel3(), activate=True, order=w.order(), rows="original")


@op("order_splat", reads=("f:density", "grid", "points", "order"), writes=("f:density",), symbols=ORDER_SPLAT + ("hns_point_order_gather",), requires=("order", "fresh_order"))
def order_splat_ranked(w, rng):
    """the per-point arrays in sorted order; float fields only, so the look-ahead memo stays"""
    o = w.order()
    torch = _torch()
    gx, ga = o.gather(w.xyz), o.gather(w.attr)
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = w.sim.splat({"density": ga}, gx, None, activate=False, status=True, rejected=rejected, order=o, rows="ranked", kernel="radial", mode="average", radius=1.5,
                         min_weight=0.125)
    return {"status": status.cpu().numpy(), "rejected": int(rejected.item())}


def _select_compact(w, fill):
    """ONE compound step, because the slots are not state: trace with status, select from it, compact both point arrays"""
    status = w.sim.trace(w.xyz, dt=DT, voxel_size=VS, order=1, steps=1, status=True)
    p = w.population()
    p.select(status)
    slot = p.slot.cpu().numpy()
    w.xyz = p.compact(w.xyz, w.xyz.clone(), fill=float("nan") if fill else None)
    w.attr = p.compact(w.attr, w.attr.clone(), fill=0 if fill else None)
    counts = p.counts()
    w.live = counts[0]
    return {"status": status.cpu().numpy(), "slot": slot, "counts": counts}


POPULATION = ("hns_sim_trace_points", "hns_point_population_select", "hns_point_population_compact", "hns_point_population_get", "hns_point_population_counts")


@op("select_compact", reads=("vel", "grid", "points"), writes=("points", "live"), symbols=POPULATION)
def select_compact_fill(w, rng):
    return _select_compact(w, True)


@op("select_compact", reads=("vel", "grid", "points"), writes=("points", "live"), symbols=POPULATION)
def select_compact_keep(w, rng):
    return _select_compact(w, False)


def _trace_collide(w, mode, order, steps, **spec):
    """the sim is only read (include/hns.h): the current velocity buffer, whichever role it plays after the calls before, and collision_sdf as it stands; a pending
    look-ahead memo is neither read nor disturbed"""
    status, hit = w.sim.trace(w.xyz, dt=DT, voxel_size=VS, order=order, steps=steps, status=True, collide=mode, hit=True, **spec)
    return status, {"status": status.cpu().numpy(), "hit": hit.cpu().numpy()}


COLLIDE_READS = ("vel", "grid", "points", "f:collision_sdf")
COLLIDE = ("hns_sim_trace_points_collide",)
COLLIDE_SPECS = {"trace_collide_stop": ("stop", 2, 2, {}), "trace_collide_push": ("push", 4, 3, dict(iterations=2, skin=1 / 16)), "trace_collide_kill_compact": ("kill", 1, 1, {})}


@op("trace_collide", reads=COLLIDE_READS, writes=("points",), symbols=COLLIDE, needs=("collision_sdf",))
def trace_collide_stop(w, rng):
    return _trace_collide(w, *COLLIDE_SPECS["trace_collide_stop"][:3])[1]


@op("trace_collide", reads=COLLIDE_READS, writes=("points",), symbols=COLLIDE, needs=("collision_sdf",))
def trace_collide_push(w, rng):
    mode, order, steps, spec = COLLIDE_SPECS["trace_collide_push"]
    return _trace_collide(w, mode, order, steps, **spec)[1]


@op("trace_collide", reads=COLLIDE_READS, writes=("points", "live"), symbols=COLLIDE + POPULATION[1:], needs=("collision_sdf",))
def trace_collide_kill_compact(w, rng):
    """ONE compound step, as _select_compact is (the slots are not state): a kill trace, select from its status, compact both point arrays with select_compact_fill's fills"""
    status, out = _trace_collide(w, *COLLIDE_SPECS["trace_collide_kill_compact"][:3])
    p = w.population()
    p.select(status, 1)
    out["slot"] = p.slot.cpu().numpy()
    w.xyz = p.compact(w.xyz, w.xyz.clone(), fill=float("nan"))
    w.attr = p.compact(w.attr, w.attr.clone(), fill=0)
    out["counts"] = p.counts()
    w.live = out["counts"][0]
    return out


CELL_READS = ("grid", "order", "cells")
VOXEL_ORDER = ("order", "fresh_order", "voxel_order")


def _neighbours(w, xyz, **kw):
    return {k: v.cpu().numpy() for k, v in w.order().neighbours(xyz, **kw).items()}


@op("neighbours", reads=("grid", "points", "order", "cells"), writes=("cells",), symbols=("hns_point_order_neighbours",), requires=VOXEL_ORDER)
def neighbours_original(w, rng):
    """radius 2: five cells an axis, the 32-lane group; the first query behind a sort builds the cell table, every later one reads it"""
    return _neighbours(w, w.xyz, radius=2.0, rows="original")


@op("neighbours", reads=("grid", "points", "order", "cells"), writes=("cells",), symbols=("hns_point_order_neighbours", "hns_point_order_gather"), requires=VOXEL_ORDER)
def neighbours_ranked(w, rng):
    """radius 0.5: two cells an axis, the 4-lane group, on the gathered positions; no density"""
    return _neighbours(w, w.order().gather(w.xyz), radius=0.5, rows="ranked", density=False)


@op("cells", reads=CELL_READS, writes=("cells",), symbols=("hns_point_order_cells",), requires=VOXEL_ORDER)
def cell_table(w, rng):
    """the whole table, and `inside` next to it (leaf_start[leaves]: the table's last entry by definition)"""
    o = w.order()
    return {"cell_start": o.cell_start.cpu().numpy(), "inside": int(o.leaf_start[w.sim.grid.leaf_count()].item())}


@op("set_live", writes=("live",), symbols=("hns_point_population_set_live", "hns_point_population_counts"))
def set_live(w, rng):
    p = w.population()
    p.set_live(int(rng.integers(N_POINTS // 4, N_POINTS // 2)))
    counts = p.counts()
    w.live = counts[0]
    return {"counts": counts}


def _birth(w, rng, append, fill, **spec):
    torch = _torch()
    p = w.population()
    voxel = torch.full((N_POINTS,), -7, dtype=torch.int32, device="cuda")
    w.sim.birth(p, "density", w.xyz, voxel, seed=_seed(rng) & 0xFFFF, append=append, fill=fill, use_masks=True, **spec)
    counts = p.counts()
    before, w.live = w.live, counts[0]
    return {"voxel": voxel.cpu().numpy(), "counts": counts, "live_before": before if append else 0}


BIRTH = ("hns_point_population_birth_sim", "hns_point_population_counts")
FEW = dict(threshold=1.5, rate=0.6, max_per_voxel=2)
MANY = dict(threshold=0.0, rate=3.0, max_per_voxel=4)  # thousands of births: more than the rows


@op("birth", reads=("f:density", "masks", "grid", "points"), writes=("points", "live"), symbols=BIRTH)
def birth(w, rng):
    """from row 0; the rows behind the births keep their positions (fill off), so the script's point set does not die with a quiet field"""
    return _birth(w, rng, False, False, **FEW)


@op("birth", reads=("f:density", "masks", "grid", "live", "points"), writes=("points", "live"), symbols=BIRTH)
def birth_append(w, rng):
    return _birth(w, rng, True, False, **FEW)


@op("birth", reads=("f:density", "masks", "grid", "live", "points"), writes=("points", "live"), symbols=BIRTH)
def birth_overflow(w, rng):
    """appended, filled, and more births than rows: wanted > live"""
    return _birth(w, rng, True, True, **MANY)


@op("solve_method", writes=("solve_method",), symbols=("hns_sim_set_solve_method",))
def method_sor(w, rng):
    w.set_method(None)
    return {}


@op("solve_method", reads=("grid",), writes=("solve_method",), symbols=("hns_sim_set_solve_method", "hns_sim_solve_levels"))
def method_vcycle_a(w, rng):
    w.set_method((2, 2, 8, 0, 1.0))
    return {"solve_levels": np.array(w.sim.solve_levels(), dtype=np.int64)}


@op("solve_method", reads=("grid",), writes=("solve_method",), symbols=("hns_sim_set_solve_method", "hns_sim_solve_levels"))
def method_vcycle_b(w, rng):
    w.set_method((1, 1, 4, 2, 1.2))
    return {"solve_levels": np.array(w.sim.solve_levels(), dtype=np.int64)}


@op("solve_control", writes=("solve_control",), symbols=("hns_sim_set_solve_control",))
def control_off(w, rng):
    w.set_control(None)
    return {}


@op("solve_control", writes=("solve_control",), symbols=("hns_sim_set_solve_control", "hns_sim_solve_report"))
def control_on(w, rng):
    """the report itself comes out of the next solve's step (a report needs a controlled solve on the same sim)"""
    w.set_control((0.5, 0.0, 2))
    return {}


@op("set_splat_spec", writes=("splat_spec",), symbols=("hns_sim_set_splat_spec", "hns_sim_get_splat_spec"))
def spec_radial_average(w, rng):
    w.set_spec((1, 1, 1.5, 0.25))
    return {}


@op("set_splat_spec", writes=("splat_spec",), symbols=("hns_sim_set_splat_spec", "hns_sim_get_splat_spec"))
def spec_default(w, rng):
    w.set_spec(DEFAULT_SPEC)
    return {}


# -- shaping (include/hns.h, SHAPING A SIM): one launch over the leaves whatever the masks say; the memo goes when the amplitude is non-zero and stays behind a decay alone


def _turbulence(rng, **control):
    return dict(amplitude=2.0, frequency=1.0 / 8, offset=tuple(float(F(c)) for c in rng.uniform(-64.0, 64.0, 3)), octaves=int(rng.integers(2, 4)), lacunarity=2.0, gain=0.5,
                seed=_seed(rng), **control)


CONTROL = dict(control="density", control_lo=-0.25, control_hi=0.75)  # the fields of these scripts are of order 1: values fall below, inside and above
DECAY = {"density": (2.0, 0.125)}
SHAPE = ("hns_shaping_apply",)


@op("shape", reads=("vel", "grid"), writes=("vel",), symbols=SHAPE, memo="drop")
def shape_turbulence(w, rng):
    w.shaping.apply(w.sim, DT, _turbulence(rng))
    return {}


@op("shape", reads=("vel", "grid", "f:density"), writes=("vel", "f:density"), symbols=SHAPE, needs=("density",), memo="drop")
def shape_controlled(w, rng):
    """the weight comes from density before this call's decay of it"""
    w.shaping.apply(w.sim, DT, _turbulence(rng, **CONTROL), DECAY)
    return {}


@op("shape", reads=("grid", "f:density"), writes=("f:density",), symbols=SHAPE, needs=("density",))
def shape_decay(w, rng):
    """amplitude 0: the velocity is neither read nor written, and what was looked ahead stays"""
    w.shaping.apply(w.sim, DT, dict(_turbulence(rng), amplitude=0.0), DECAY)
    return {}


# -- diffusion (DIFFUSING A SIM): the iterates ping-pong in the sim's adv, tmp and nxt buffers and in ONE block the object keeps between calls; only the unknowns are written


def coefficient_of(a):
    """the coefficient that gives a = coefficient * DT / VS^2"""
    return a * VS * VS / DT


# name -> ({field: a}, the velocity's a, iterations, method, collide): 1, 5, 0 and 1 written float fields, so the object's block is carved anew from call to call
DIFFUSE_SPECS = {
    "diffuse_copy": ({"density": 0.5}, 0.0, 1, "jacobi", False),
    "diffuse_fields": (dict(zip(fc.COMBUST, (0.05, 0.3, 1.0, 2.0, 4.0))), 0.0, 3, "chebyshev", False),
    "diffuse_viscosity": ({}, 1.5, 2, "jacobi", False),
    "diffuse_walls": ({"density": 4.0}, 0.75, 4, "chebyshev", True),
}
DIFFUSE = ("hns_diffusion_apply",)


def diffuse_arguments(name):
    """the keywords of Diffusion.apply (and of diffusion_cases.apply_mirror) of a diffuse operation"""
    fields, viscosity, iterations, method, collide = DIFFUSE_SPECS[name]
    return dict(fields={k: coefficient_of(a) for k, a in fields.items()}, viscosity=coefficient_of(viscosity), iterations=iterations, method=method, collide=collide, threshold=0.0)


def _diffuse(w, name):
    w.diffusion.apply(w.sim, DT, VS, **diffuse_arguments(name))
    return {}


@op("diffuse", reads=("grid", "masks", "f:density"), writes=("f:density",), symbols=DIFFUSE, needs=("density",))
def diffuse_copy(w, rng):
    """iterations == 1: the one iterate lies in the scratch and a copy brings it into the field"""
    return _diffuse(w, "diffuse_copy")


@op("diffuse", reads=("grid", "masks") + ADVECTED, writes=ADVECTED, symbols=DIFFUSE, needs=fc.COMBUST)
def diffuse_fields(w, rng):
    return _diffuse(w, "diffuse_fields")


@op("diffuse", reads=("grid", "masks", "vel"), writes=("vel",), symbols=DIFFUSE, memo="drop")
def diffuse_viscosity(w, rng):
    return _diffuse(w, "diffuse_viscosity")


@op("diffuse", reads=("grid", "masks", "vel", "f:density", "f:collision_sdf"), writes=("vel", "f:density"), symbols=DIFFUSE, needs=("density", "collision_sdf"), memo="drop")
def diffuse_walls(w, rng):
    return _diffuse(w, "diffuse_walls")


# -- points with a velocity of their own (POINTS WITH A VELOCITY OF THEIR OWN): the sim is only read, the object is bound to no grid

GRAVITY = (0.0, -9.8, 0.0)
# name -> (mode, steps or None = 1 .. 3 from the step's rng, the keywords of PointMotion.step); the ages are drawn in [0, 1), so a finite max_age below 1 expires rows
MOTION_SPECS = {
    "motion_free": ("free", 1, dict(gravity=GRAVITY, drag=2.0)),
    "motion_stick": ("stick", None, dict(gravity=GRAVITY, drag=1.0, max_age=0.9)),
    "motion_bounce": ("bounce", None, dict(gravity=GRAVITY, drag=2.0, restitution=0.5, friction=0.25, max_age=0.95, skin=1 / 16, iterations=3)),
    "motion_kill_compact": ("kill", 1, dict(gravity=GRAVITY, drag=2.0, max_age=0.9)),
}
MOTION = ("hns_point_motion_step", "hns_point_motion_get")
MOTION_READS = ("vel", "grid", "motion")


@op("motion_load", reads=("points",), writes=("motion",), symbols=("hns_point_motion_get",))
def motion_load(w, rng):
    """points -> motion: through the device pointers the object hands out"""
    w.motion.xyz.copy_(w.xyz)
    w.motion.vel.copy_(w.vel3())
    w.motion.age.copy_(_torch().from_numpy(rng.random(N_POINTS).astype(F)).cuda())
    return {}


@op("motion_store", reads=("motion",), writes=("points",), symbols=("hns_point_motion_get",))
def motion_store(w, rng):
    """motion -> points: the sorts, splats, traces and queries behind it read the moved positions"""
    w.xyz = w.motion.xyz.clone()
    return {}


def _motion(w, rng, name):
    mode, steps, spec = MOTION_SPECS[name]
    steps = int(rng.integers(1, 4)) if steps is None else steps
    w.motion.step(w.sim, N_POINTS, DT, VS, steps, mode, **spec)
    return {"status": w.motion.status.cpu().numpy(), "hit": w.motion.hit.cpu().numpy(), "steps": steps}


@op("motion", reads=MOTION_READS, writes=("motion",), symbols=MOTION)
def motion_free(w, rng):
    return _motion(w, rng, "motion_free")


@op("motion", reads=MOTION_READS + ("f:collision_sdf",), writes=("motion",), symbols=MOTION, needs=("collision_sdf",))
def motion_stick(w, rng):
    return _motion(w, rng, "motion_stick")


@op("motion", reads=MOTION_READS + ("f:collision_sdf",), writes=("motion",), symbols=MOTION, needs=("collision_sdf",))
def motion_bounce(w, rng):
    return _motion(w, rng, "motion_bounce")


@op("motion", reads=MOTION_READS + ("f:collision_sdf",), writes=("motion", "live"), symbols=MOTION + POPULATION[1:], needs=("collision_sdf",))
def motion_kill_compact(w, rng):
    """ONE compound step, as trace_collide_kill_compact is (the slots are not state): a kill step, select from its status, compact xyz, vel and age into the motion's arrays"""
    out = _motion(w, rng, "motion_kill_compact")
    m, p = w.motion, w.population()
    p.select(m.status, 1)
    out["slot"] = p.slot.cpu().numpy()
    for a, fill in ((m.xyz, float("nan")), (m.vel, 0.0), (m.age, 0.0)):
        p.compact(a.clone(), a, fill=fill)
    out["counts"] = p.counts()
    w.live = out["counts"][0]
    return out


KINDS = tuple(dict.fromkeys(o.kind for o in OPS.values()))
PRODUCERS = frozenset(k for k, o in OPS.items() if o.memo == "produce")

# ---- conditions on scripts, from the table alone (no device) ---------------------------------------------------------------------------------------------------------


class Script(NamedTuple):
    name: str
    profile: str
    seed: int
    timing: bool
    steps: tuple  # of (operation name, seed)

    @property
    def ops(self):
        return [OPS[k] for k, _ in self.steps]


def profile_allows(profile, operation: Op):
    return operation.needs <= set(PROFILES[profile])


def depends(a: Op, b: Op):
    """what `a` writes that `b` reads, or that a memo `b` consumes depends on"""
    return a.writes & b.reads


def feasible(a: Op, b: Op):
    """can `b` directly follow `a` in some script? not when `a` breaks what `b` requires of the steps before it"""
    return not (a.breaks & b.requires) and any(profile_allows(p, a) and profile_allows(p, b) for p in PROFILES)


def needed_pairs():
    """{(kind A, kind B): [(a, b) operation names that would cover it]}"""
    out = {}
    for ka, a in OPS.items():
        for kb, b in OPS.items():
            if depends(a, b) and feasible(a, b):
                out.setdefault((a.kind, b.kind), []).append((ka, kb))
    return out


def covered_pairs(scripts):
    out = {}
    for s in scripts:
        for i in range(1, len(s.steps)):
            a, b = OPS[s.steps[i - 1][0]], OPS[s.steps[i][0]]
            if depends(a, b):
                out.setdefault((a.kind, b.kind), []).append((s.name, i))
    return out


def placed_writers():
    """the operations that must sit between two look-ahead substeps in some script: every writer of the velocity, every change of grid and everything else that drops
    the memo -- but the substeps that leave a memo themselves"""
    return [k for k, o in OPS.items() if k not in PRODUCERS and ("vel" in o.writes or o.grid or o.memo == "drop")]


def placements(scripts):
    out = {}
    for s in scripts:
        names = [k for k, _ in s.steps]
        for i in range(1, len(names) - 1):
            if names[i - 1] in PRODUCERS and names[i + 1] in PRODUCERS:
                out.setdefault(names[i], []).append((s.name, i))
    return out


class Tracker:
    """what a script has established so far, as far as the table can tell: is there an order on the current grid, does it match the positions, and is it by voxel?"""

    def __init__(self):
        self.have = set()

    def refusal(self, profile, name):
        o = OPS[name]
        if not profile_allows(profile, o):
            return f"{name} needs the fields {sorted(o.needs)}, the profile {profile} holds {PROFILES[profile]}"
        if not o.requires <= self.have:
            return (f"{name} requires {sorted(o.requires - self.have)}: a sort since the last change of grid (fresh_order: and since the last write of the positions; "
                    f"voxel_order: and the last sort by voxel)")
        return None

    def step(self, name):
        o = OPS[name]
        self.have -= o.breaks
        self.have |= o.sets


def refusals(script: Script):
    """the steps of a script the library (or its Python objects) would refuse, by the table"""
    t, out = Tracker(), []
    for i, (name, _) in enumerate(script.steps):
        if name not in OPS:
            out.append((i, f"{name} is no operation"))
            continue
        why = t.refusal(script.profile, name)
        if why:
            out.append((i, why))
        t.step(name)
    return out


def expected_lookahead(script: Script, upto=None):
    """(produced, consumed) after every step under lookahead = 1, by the table's memo column"""
    live, produced, consumed, out = False, 0, 0, []
    for o in script.ops[:upto]:
        if o.memo in ("produce", "consume"):
            consumed += live
            live = o.memo == "produce"
            produced += live
        elif o.memo == "drop":
            live = False
        out.append((produced, consumed))
    return out


def has_two_equal_substeps(script: Script):
    names = [k for k, _ in script.steps]
    return any(a in PRODUCERS and b in PRODUCERS for a, b in zip(names, names[1:]))


# ---- the generator the committed scripts were drawn with ---------------------------------------------------------------------------------------------------------------


def draw_scripts(seed=2026, max_steps=24, max_scripts=16, only=None, first_seed=101):
    """Placement scripts first (substep, writer, substep, writer, ...), then greedy walks that take the step covering the most uncovered pairs. Prints nothing; returns the
    scripts, whose text (`format_scripts`) is pasted below. The CPU test holds the conditions on the committed text, not on this function.
    only: a set of pairs of kinds -- no placement scripts, and the walks go for these pairs alone (what a grown table adds to the committed scripts)"""
    rng = np.random.default_rng(seed)
    ways_of = needed_pairs()
    need = set(ways_of) if only is None else set(only) & set(ways_of)
    scripts, counter = [], [first_seed - 1]

    def next_seed():
        counter[0] += 1
        return counter[0]

    def finish(name, profile, names, timing=False):
        s = Script(name, profile, next_seed(), timing, tuple((k, next_seed()) for k in names))
        assert not refusals(s), (name, refusals(s))
        scripts.append(s)
        need.difference_update(covered_pairs([s]))

    # placement: S S w S w S ..., a sort in front of a producer where the writer needs an order
    writers = placed_writers()
    groups = {"collide": [k for k in writers if "collision_sdf" in OPS[k].needs], "one": [], "combust": []}
    rest = [k for k in writers if k not in groups["collide"]]
    for i, k in enumerate(rest):
        groups["one" if (not OPS[k].needs and i % 2) else "combust"].append(k)
    groups["collide"] += groups["combust"][-3:]
    del groups["combust"][-3:]
    for profile, ws in groups.items() if only is None else ():
        cycle = ["core_substep"] if profile == "one" else ["core_substep", "substep_unfused"]
        names, t = [cycle[0]], Tracker()
        for j, k in enumerate(ws):
            if t.refusal(profile, k):
                names += ["sort_voxel" if j % 2 else "sort_leaf", cycle[j % len(cycle)]]
                t.step(names[-2])
            names += [k, cycle[(j + 1) % len(cycle)]]
            t.step(k)
        finish(f"placement_{profile}", profile, [cycle[-1]] + names, timing=profile == "combust")

    # greedy walks
    profiles = ["combust", "collide", "one", "combust"]
    while need and len(scripts) < max_scripts:
        profile = profiles[len(scripts) % len(profiles)]
        names, t, idle = [], Tracker(), 0

        def gain(a, b):
            return 1.0 if (OPS[a].kind, OPS[b].kind) in need and depends(OPS[a], OPS[b]) else 0.0

        while len(names) < max_steps:
            best, best_score = None, 0.0
            for k in rng.permutation(list(OPS)):
                k, o = str(k), OPS[str(k)]
                if t.refusal(profile, k):
                    continue
                t2 = Tracker()
                t2.have = set(t.have)
                t2.step(k)
                onward = max([gain(k, c) for c in OPS if c != k and not t2.refusal(profile, c)
                              and not (names and OPS[c].kind == OPS[names[-1]].kind and o.kind == OPS[c].kind)] or [0.0])
                after = sum(1 for (a, b), ways in ways_of.items() if (a, b) in need and a == o.kind and any(x == k and profile_allows(profile, OPS[y]) for x, y in ways))
                score = (gain(names[-1], k) if names else 0.0) + 0.9 * onward + 0.01 * after
                if o.grid and sum(OPS[x].grid for x in names) >= 4:
                    score *= 0.1  # (keeps a script's domain from growing without end)
                if score > best_score:
                    best, best_score = k, score
            if best is None:
                break
            names.append(best)
            t.step(best)
            won = len(names) > 1 and gain(names[-2], best) > 0
            if won:
                need.discard((OPS[names[-2]].kind, OPS[best].kind))
            idle = 0 if won else idle + 1
            if idle >= 3:
                del names[-3:]
                break
        if len(names) < 6:
            break  # (the walk finds too little: the rest is picked up pair by pair)
        finish(f"walk_{len(scripts)}", profile, names, timing=len(scripts) % 5 == 0)

    # what the walks left: pair by pair, each with the sort it requires in front
    while need and len(scripts) < max_scripts:
        profile = "combust" if all(any(profile_allows("combust", OPS[a]) and profile_allows("combust", OPS[b]) for a, b in ways_of[p]) for p in need) else "collide"
        names, t = [], Tracker()
        for p in sorted(need):
            a, b = next((a, b) for a, b in ways_of[p] if profile_allows(profile, OPS[a]) and profile_allows(profile, OPS[b]))
            seg, t2 = [], Tracker()
            t2.have = set(t.have)
            if names and names[-1] == a and not t2.refusal(profile, b):
                seg = [b]
            else:
                if (OPS[a].requires | (OPS[b].requires - OPS[a].breaks)) - t2.have:
                    seg.append("sort_voxel")
                seg += [a, b]
            if len(names) + len(seg) > max_steps:
                break
            for k in seg:
                names.append(k)
                t.step(k)
        finish(f"pairs_{len(scripts)}", profile, names)
    return scripts, need


def format_scripts(scripts):
    lines = ["SCRIPTS = ("]
    for s in scripts:
        lines.append(f'    Script("{s.name}", "{s.profile}", {s.seed}, {s.timing}, (')
        row = "        "
        for k, sd in s.steps:
            item = f'("{k}", {sd}), '
            if len(row) + len(item) > 168:
                lines.append(row.rstrip())
                row = "        "
            row += item
        lines.append(row.rstrip())
        lines.append("    )),")
    lines.append(")")
    return "\n".join(lines)


# ---- the committed scripts -----------------------------------------------------------------------------------------------------------------------------------------------

# the first twelve were drawn by draw_scripts on the table as it stood before collision tracing and the neighbourhoods joined it (its closing three-step script folded
# into frame_vcycle); they and their seeds stay as they are. frame_vcycle is written by hand: a V-cycle method and a control on a sim, then a seeded regrid, an ordered
# splat of the velocity, substeps, a deactivate, statistics, a birth from a field, a regrid onto another leaf count, a stored spec set and put back, and the way back to
# SOR -- and the operations no drawn script of that table holds. The last three are written by hand too, for the pairs the two features add (POINT_SCRIPTS below).
SCRIPTS = (
    Script("placement_collide", "collide", 101, False, (
        ("substep_unfused", 102), ("core_substep", 103), ("substep_collision", 104), ("substep_unfused", 105), ("regrid_sdf", 106), ("core_substep", 107),
        ("deactivate", 108), ("substep_unfused", 109), ("splat_velocity", 110), ("core_substep", 111), ("splat_stored", 112), ("substep_unfused", 113),
    )),
    Script("placement_one", "one", 114, False, (
        ("core_substep", 115), ("core_substep", 116), ("upload_field", 117), ("core_substep", 118), ("advect_names", 119), ("core_substep", 120),
        ("regrid_plain", 121), ("core_substep", 122), ("regrid_seeded", 123), ("core_substep", 124), ("emit_radial", 125), ("core_substep", 126),
        ("deactivate_counts", 127), ("core_substep", 128), ("splat_both", 129), ("core_substep", 130), ("sort_voxel", 131), ("core_substep", 132),
        ("order_splat_original", 133), ("core_substep", 134),
    )),
    Script("placement_combust", "combust", 135, True, (
        ("substep_unfused", 136), ("core_substep", 137), ("upload_vel", 138), ("substep_unfused", 139), ("upload_all", 140), ("core_substep", 141),
        ("substep_fused", 142), ("substep_unfused", 143), ("substep_vorticity", 144), ("core_substep", 145), ("advect_velocity", 146), ("substep_unfused", 147),
        ("regrid_sourced", 148), ("core_substep", 149), ("emit_trilinear", 150), ("substep_unfused", 151),
    )),
    Script("walk_3", "combust", 152, False, (
        ("regrid_plain", 153), ("regrid_seeded", 154), ("emit_radial", 155), ("emit_trilinear", 156), ("advect_velocity", 157), ("splat_stored", 158),
        ("splat_both", 159), ("advect_velocity", 160), ("advect_velocity", 161), ("select_compact_fill", 162), ("splat_stored", 163), ("birth", 164), ("trace", 165),
        ("trace", 166), ("splat_velocity", 167), ("select_compact_keep", 168), ("select_compact_keep", 169), ("birth_overflow", 170), ("birth_append", 171),
        ("splat_velocity", 172), ("deactivate_counts", 173), ("deactivate_counts", 174), ("splat_both", 175), ("trace", 176),
    )),
    Script("walk_4", "combust", 177, False, (
        ("regrid_plain", 178), ("substep_fused", 179), ("emit_radial", 180), ("regrid_seeded", 181), ("advect_velocity", 182), ("regrid_seeded", 183),
        ("masks_array", 184), ("birth_append", 185), ("select_compact_fill", 186), ("trace", 187), ("birth_append", 188), ("sort_voxel", 189),
        ("order_splat_original", 190), ("order_splat_original", 191), ("substep_fused", 192), ("order_splat_original", 193), ("advect_velocity", 194),
        ("order_splat_original", 195), ("trace", 196), ("gather_scatter", 197), ("gather_scatter", 198), ("splat_floats", 199), ("upload_all", 200),
        ("advect_velocity", 201),
    )),
    Script("walk_5", "collide", 202, True, (
        ("emit_trilinear", 203), ("masks_array", 204), ("regrid_seeded", 205), ("select_compact_keep", 206), ("emit_radial", 207), ("splat_velocity", 208),
        ("emit_radial", 209), ("deactivate", 210), ("birth_append", 211), ("upload_all", 212), ("trace", 213), ("select_compact_keep", 214), ("sort_voxel", 215),
        ("gather_scatter", 216), ("order_splat_original", 217), ("birth_overflow", 218), ("gather_scatter", 219), ("trace", 220), ("sort_voxel", 221),
        ("upload_all", 222), ("order_splat_original", 223), ("splat_floats", 224), ("order_splat_original", 225), ("deactivate_counts", 226),
    )),
    Script("walk_6", "one", 227, False, (
        ("regrid_plain", 228), ("deactivate_counts", 229), ("emit_trilinear", 230), ("method_vcycle_b", 231), ("regrid_plain", 232), ("splat_stored", 233),
        ("regrid_sourced", 234), ("method_vcycle_b", 235), ("core_substep", 236), ("birth_append", 237), ("sample", 238), ("upload_all", 239),
        ("select_compact_fill", 240), ("sample", 241), ("upload_field", 242), ("deactivate", 243), ("stats", 244), ("upload_all", 245), ("birth_overflow", 246),
        ("advect_velocity", 247), ("trace", 248), ("sample", 249), ("advect_names", 250), ("deactivate", 251),
    )),
    Script("walk_7", "combust", 252, False, (
        ("emit_radial", 253), ("trace", 254), ("emit_trilinear", 255), ("select_compact_fill", 256), ("regrid_seeded", 257), ("birth", 258), ("regrid_seeded", 259),
        ("trace", 260), ("substep_fused", 261), ("advect_names", 262), ("birth_overflow", 263), ("substep_unfused", 264), ("deactivate_counts", 265),
        ("masks_array", 266), ("splat_floats", 267), ("sample", 268), ("upload_all", 269), ("splat_both", 270), ("stats", 271), ("substep_vorticity", 272),
        ("trace", 273), ("substep_fused", 274), ("birth", 275), ("upload_field", 276),
    )),
    Script("walk_8", "combust", 277, False, (
        ("emit_trilinear", 278), ("birth_overflow", 279), ("emit_trilinear", 280), ("sort_leaf", 281), ("gather_scatter", 282), ("regrid_seeded", 283),
        ("sort_voxel", 284), ("gather_scatter", 285), ("emit_trilinear", 286), ("sample", 287), ("masks_none", 288), ("deactivate", 289), ("upload_all", 290),
        ("stats", 291), ("core_substep", 292), ("trace", 293), ("advect_names", 294), ("sample", 295), ("upload_field", 296), ("sample", 297), ("masks_array", 298),
        ("stats", 299), ("substep_unfused", 300), ("select_compact_fill", 301),
    )),
    Script("walk_9", "collide", 302, False, (
        ("core_substep", 303), ("select_compact_keep", 304), ("regrid_sourced", 305), ("sample", 306), ("control_on", 307), ("substep_vorticity", 308), ("stats", 309),
        ("method_vcycle_a", 310), ("emit_radial", 311), ("stats", 312), ("deactivate_counts", 313), ("regrid_plain", 314), ("pressure_residual", 315),
        ("control_off", 316), ("core_substep", 317), ("sample", 318), ("upload_all", 319), ("regrid_sourced", 320), ("stats", 321), ("method_sor", 322),
        ("substep_vorticity", 323), ("sample", 324), ("masks_array", 325), ("advect_velocity", 326),
    )),
    Script("walk_10", "one", 327, True, (
        ("advect_names", 328), ("emit_trilinear", 329), ("pressure_residual", 330), ("masks_array", 331), ("emit_trilinear", 332), ("method_vcycle_a", 333),
        ("pressure_residual", 334), ("control_on", 335), ("pressure_residual", 336), ("upload_vel", 337), ("emit_trilinear", 338), ("trace", 339),
        ("regrid_seeded", 340), ("advect_names", 341), ("stats", 342), ("core_substep", 343), ("stats", 344), ("spec_radial_average", 345), ("splat_stored", 346),
        ("set_live", 347), ("birth_append", 348),
    )),
    Script("pairs_11", "combust", 349, False, (
        ("sort_voxel", 350), ("deactivate", 351), ("order_splat_original", 352), ("gather_scatter", 353), ("birth_append", 354), ("gather_scatter", 355),
        ("sample", 356), ("gather_scatter", 357), ("select_compact_fill", 358), ("gather_scatter", 359), ("sort_voxel", 360), ("order_splat_original", 361),
        ("emit_trilinear", 362), ("sort_voxel", 363), ("order_splat_original", 364), ("regrid_plain", 365), ("sort_voxel", 366), ("order_splat_original", 367),
        ("sample", 368), ("order_splat_original", 369), ("select_compact_fill", 370), ("sort_voxel", 371), ("order_splat_original", 372), ("stats", 373),
    )),
    Script("frame_vcycle", "combust", 374, True, (
        ("method_vcycle_a", 375), ("control_on", 376), ("regrid_seeded", 377), ("sort_voxel", 378), ("masks_array", 379), ("order_splat_original", 380),
        ("core_substep", 381), ("core_substep", 382), ("deactivate", 383), ("stats", 384), ("birth", 385), ("substep_unfused", 386), ("substep_unfused", 387),
        ("regrid_plain", 388), ("pressure_residual", 389), ("method_vcycle_b", 390), ("spec_radial_average", 391), ("splat_stored", 392), ("spec_default", 393),
        ("splat_stored", 394), ("control_off", 395), ("method_sor", 396), ("core_substep", 397), ("sort_leaf", 398), ("order_splat_ranked", 399), ("core_substep", 400),
    )),
)

# Written by hand, all three on a sim that holds collision_sdf.
#   collide_points  every call kind that writes what the collision trace reads (the velocity, the fields, the grid, the positions) directly in front of one, and every
#                   kind that reads the positions directly behind one: upload, regrid, emit, splat, select, birth, trace, advect, and a trace behind a trace.
#   cells_memo      the order's cell table through its transitions on ONE order object: built by a query behind a sort, read again by the table's download, twice, by
#                   a query at another radius (another k_neighbours<G>), behind a gather / scatter; a sort by voxel, by leaf and by voxel again in front of a query;
#                   a query behind an ordered splat's trace and gather / scatter; the table built by its download instead of by a query; a kill in front of a sort.
#   frame_points    the frame loop the two features were built for: a push under a pending look-ahead memo that the next substep consumes, a kill that drops rows, the
#                   sort, the queries at both radii around an ordered splat, a regrid (a new order object), a sort by leaf then by voxel, the table, a collision substep
#                   and a stop.
# What the twin showed on the MI355X (check_liveness of tests/test_sequences_gpu.py prints it) stands above each script.
POINT_SCRIPTS = (
    # twin: rows (hit == 0, hit != 0) of the nine traces (793, 707) (756, 744) (1427, 73) (1312, 188) (1422, 78) (1419, 81) (1458, 42) (1489, 11) (1397, 103); rows with
    # the mode's bit: stop put back 789, push pushed 1062 and put back 58, kill killed 76; the kill kept 1424 of 1500; 1220 leaves at the end
    Script("collide_points", "collide", 401, False, (
        ("upload_all", 402), ("trace_collide_stop", 403), ("regrid_seeded", 404), ("trace_collide_push", 405), ("emit_trilinear", 406), ("trace_collide_stop", 407),
        ("splat_both", 408), ("trace_collide_push", 409), ("select_compact_keep", 410), ("trace_collide_stop", 411), ("birth_append", 412),
        ("trace_collide_kill_compact", 413), ("trace", 414), ("trace_collide_push", 415), ("trace_collide_stop", 416), ("sample", 417), ("advect_velocity", 418),
        ("trace_collide_push", 419),
    )),
    # twin: traces (827, 673) (775, 725) (1438, 62); stop put back 595, push pushed 707 and put back 17, kill killed 61, kept 297 of 1500; rows (count == 0, count != 0)
    # of the six queries (874, 626) (1451, 49) (874, 626) (1451, 49) (1308, 192) (1459, 41); table entries strictly between 0 and inside, and inside: (15839, 878) twice,
    # (15798, 363); 31 leaves throughout
    Script("cells_memo", "collide", 420, True, (
        ("birth_overflow", 421), ("sort_voxel", 422), ("neighbours_original", 423), ("cell_table", 424), ("cell_table", 425), ("neighbours_ranked", 426),
        ("gather_scatter", 427), ("neighbours_original", 428), ("sort_voxel", 429), ("sort_leaf", 430), ("sort_voxel", 431), ("neighbours_ranked", 432),
        ("order_splat_original", 433), ("trace_collide_stop", 434), ("gather_scatter", 435), ("trace_collide_push", 436), ("sort_voxel", 437), ("cell_table", 438),
        ("neighbours_original", 439), ("trace_collide_kill_compact", 440), ("sort_voxel", 441), ("neighbours_ranked", 442),
    )),
    # twin: traces (826, 674) (1450, 50) (1478, 22); push pushed 631 and put back 16, kill killed 50, kept 410 of 1500, stop put back 21; queries (1299, 201)
    # (1457, 43) (1299, 201) (1457, 43); table (236450, 410); look-ahead counts (3, 2) under lookahead = 1; 498 leaves at the end. Against the mirrors: the push moved 1048
    # rows, no word differs; the first query finds 350 pairs among the 410 points that take part
    Script("frame_points", "collide", 443, False, (
        ("core_substep", 444), ("core_substep", 445), ("trace_collide_push", 446), ("core_substep", 447), ("trace_collide_kill_compact", 448), ("sort_voxel", 449),
        ("neighbours_original", 450), ("neighbours_ranked", 451), ("order_splat_original", 452), ("neighbours_original", 453), ("regrid_sdf", 454), ("sort_leaf", 455),
        ("sort_voxel", 456), ("cell_table", 457), ("neighbours_ranked", 458), ("substep_collision", 459), ("trace_collide_stop", 460),
    )),
)
SCRIPTS += POINT_SCRIPTS

# The three features merged since: points with a velocity of their own, shaping, diffusion. The first three are written by hand, the last four drawn by draw_scripts(only=
# the pairs the three left uncovered) and touched up by hand (a masks_array or a deactivate in front, so that no diffuse runs with every voxel an unknown of random values).
#   frame_shaped   the frame loop the features were built for: a controlled shape and a diffuse with walls between two substeps, points loaded into the motion, bounced,
#                  killed and compacted, stored back, sorted and splatted through the order; a regrid; and the same again on the new grid, through the SAME PointMotion,
#                  Shaping and Diffusion.
#   memo_kept      every shape and diffuse directly between two look-ahead substeps: shape_decay, diffuse_copy and diffuse_fields must leave the memo for the next substep
#                  to consume, the four that write the velocity must drop it. On the one Diffusion the written float fields go 1, 5, (1), 0, 1 and, behind a regrid onto
#                  a larger grid, 0 and 5: its block is carved anew and drawn anew. A diffuse of the velocity (adv, tmp) in front of the vorticity stage.
#   motion_regrid  motion steps either side of a regrid and of an emit with no load between them: the one object follows the sim onto its new grids; a store in front of
#                  a collision trace, a kill in front of a store and a birth; deactivate in front of a diffuse; a collision substep in front of a stick.
# What the twin showed on the MI355X (check_liveness of tests/test_sequences_gpu.py prints it) stands above each script.
FEATURE_SCRIPTS = (
    # twin: 31 leaves, 525 behind the regrid. Control (below, inside, above) of the two shapes (6174, 7249, 1425) (4691, 263983, 126); the diffuses changed 30752 of 59392
    # words with 7119 solid voxels and 7729 unknowns, then 111419 of 1075200 with 240161 of 268800 voxels inactive, 2038 solid, 27902 unknowns. Bounces: status (0, 1)
    # (1118, 382) and (1344, 156), rows per hit bit 1, 8, 16: 438, 529, 203 and 5, 3, 4; the kills killed 200 and 2, kept 171 and 134 of 1500; 414 rows expired by age.
    # look-ahead counts (4, 0) under lookahead = 1. Against the mirrors (3 octaves; 1 bounce step): no word differs in any of the three
    Script("frame_shaped", "collide", 461, False, (
        ("core_substep", 462), ("shape_controlled", 463), ("diffuse_walls", 464), ("core_substep", 465), ("motion_load", 466), ("motion_bounce", 467),
        ("motion_kill_compact", 468), ("motion_store", 469), ("sort_voxel", 470), ("order_splat_original", 471), ("regrid_sdf", 472), ("core_substep", 473),
        ("shape_controlled", 474), ("diffuse_walls", 475), ("core_substep", 476), ("motion_load", 477), ("motion_bounce", 478), ("motion_kill_compact", 479),
        ("motion_store", 480), ("sort_voxel", 481), ("order_splat_original", 482),
    )),
    # twin: 9282 of 14848 voxels inactive from the first step on, 160868 of 177152 behind the regrid (31 -> 346 leaves). Words changed: copy 5384 of 14848, fields 26828 of
    # 74240, viscosity 16152 of 44544, walls 11219 of 59392 (6994 solid, 2888 unknowns); on the larger grid viscosity 48642 of 531456, fields 70067 of 885760. The decay
    # moved no velocity word and all 14848 of density; control (890, 13836, 122). look-ahead counts (10, 4) under lookahead = 1: the three keeps were each consumed behind
    Script("memo_kept", "collide", 483, True, (
        ("masks_array", 484), ("core_substep", 485), ("substep_unfused", 486), ("shape_decay", 487), ("core_substep", 488), ("diffuse_copy", 489),
        ("substep_unfused", 490), ("diffuse_fields", 491), ("core_substep", 492), ("shape_turbulence", 493), ("substep_unfused", 494), ("shape_controlled", 495),
        ("core_substep", 496), ("diffuse_viscosity", 497), ("substep_unfused", 498), ("diffuse_walls", 499), ("core_substep", 500), ("regrid_plain", 501),
        ("diffuse_viscosity", 502), ("substep_vorticity", 503), ("diffuse_fields", 504), ("core_substep", 505),
    )),
    # twin: sticks of 3, 3 and 1 steps, status (0, 1) (1084, 416) (1009, 491) (323, 1177), stuck 608, 613, 407, started inside 467, 195, 457; bounces of 2 and 3 steps
    # (1175, 325) (1185, 315), bounced 609 and 149, reflected 453 and 91, put back 1; the kill killed 38 and kept 563 of 1500; 2906 rows expired by age over the script.
    # diffuse_copy behind the deactivate: 462841 of 472064 voxels inactive, 9024 words changed; walls 86601 of 1046528 (7388 solid, 22518 unknowns). 511 leaves at the end
    Script("motion_regrid", "collide", 506, False, (
        ("motion_load", 507), ("motion_free", 508), ("motion_stick", 509), ("regrid_seeded", 510), ("motion_stick", 511), ("motion_bounce", 512),
        ("emit_trilinear", 513), ("motion_bounce", 514), ("motion_store", 515), ("trace_collide_stop", 516), ("motion_load", 517), ("motion_kill_compact", 518),
        ("motion_store", 519), ("birth_append", 520), ("motion_load", 521), ("motion_free", 522), ("deactivate", 523), ("diffuse_copy", 524), ("regrid_plain", 525),
        ("diffuse_walls", 526), ("deactivate_counts", 527), ("shape_decay", 528), ("substep_collision", 529), ("motion_stick", 530),
    )),
    # twin: seven controlled shapes, the control (5820, 6113, 3427) at first and (4403, 844093, 1424) on the last grid; four viscosity diffuses under masks with 7610 of
    # 15360 and then 397614 of 451072 voxels inactive, 23082 of 46080 and 94646 of 1353216 words changed. 1660 leaves at the end
    Script("walk_19", "combust", 531, True, (
        ("masks_array", 532), ("shape_controlled", 533), ("shape_controlled", 534), ("splat_stored", 535), ("diffuse_viscosity", 536), ("diffuse_viscosity", 537),
        ("shape_controlled", 538), ("advect_velocity", 539), ("diffuse_viscosity", 540), ("splat_stored", 541), ("shape_controlled", 542), ("emit_trilinear", 543),
        ("diffuse_viscosity", 544), ("advect_velocity", 545), ("shape_controlled", 546), ("regrid_seeded", 547), ("shape_controlled", 548), ("trace", 549),
        ("motion_load", 550), ("motion_store", 551), ("emit_radial", 552), ("shape_controlled", 553), ("select_compact_fill", 554), ("motion_load", 555),
    )),
    # twin: five diffuses with walls, 7519 solid voxels throughout, 8353 unknowns on the first grid and 88636 of 483328 voxels behind the emit; kills killed 435 and 126 (489
    # rows started inside), kept 329 and 192 of 1500, 158 rows expired; control (3361, 478294, 1673) and (2891, 478878, 1559). 944 leaves at the end
    Script("walk_20", "collide", 556, False, (
        ("diffuse_walls", 557), ("motion_kill_compact", 558), ("birth_append", 559), ("diffuse_walls", 560), ("emit_radial", 561), ("motion_store", 562),
        ("splat_both", 563), ("motion_kill_compact", 564), ("diffuse_walls", 565), ("select_compact_keep", 566), ("shape_controlled", 567),
        ("trace_collide_stop", 568), ("motion_store", 569), ("sample", 570), ("diffuse_walls", 571), ("sample", 572), ("motion_store", 573),
        ("select_compact_fill", 574), ("shape_controlled", 575), ("birth_append", 576), ("diffuse_walls", 577), ("birth_append", 578), ("motion_store", 579),
        ("motion_load", 580),
    )),
    # twin: no collision_sdf in this profile: motion_free alone, status (0, 1) (778, 722) (92, 1408) (168, 1332) (273, 1227), no hit bit. Viscosity under the deactivate's masks
    # (6849 of 15872 voxels inactive): 26672 and 26698 of 47616 words changed; the copy behind masks_none, every voxel an unknown: 33576 of 263168. 514 leaves at the end
    Script("walk_21", "one", 581, False, (
        ("shape_controlled", 582), ("deactivate", 583), ("upload_vel", 584), ("shape_controlled", 585), ("motion_free", 586), ("motion_store", 587), ("trace", 588),
        ("diffuse_viscosity", 589), ("stats", 590), ("upload_all", 591), ("diffuse_viscosity", 592), ("trace", 593), ("shape_controlled", 594), ("sample", 595),
        ("motion_store", 596), ("regrid_seeded", 597), ("core_substep", 598), ("motion_free", 599), ("masks_none", 600), ("diffuse_copy", 601), ("upload_vel", 602),
        ("motion_free", 603), ("advect_velocity", 604), ("motion_free", 605),
    )),
    # twin: copies under the deactivate's masks and the ordered splats' activations: 9365 and 11756 of 15872 words changed (6408, then 4084 voxels inactive), viscosity 34338
    # of 47616; motion_free status (0, 1) (809, 691); the stop put back 582; control (4617, 10238, 1017). 31 leaves throughout
    Script("pairs_22", "collide", 606, False, (
        ("deactivate", 607), ("sort_voxel", 608), ("diffuse_copy", 609), ("order_splat_original", 610), ("diffuse_viscosity", 611), ("trace_collide_stop", 612),
        ("gather_scatter", 613), ("motion_load", 614), ("motion_store", 615), ("gather_scatter", 616), ("sort_voxel", 617), ("order_splat_original", 618),
        ("diffuse_copy", 619), ("order_splat_original", 620), ("motion_free", 621), ("order_splat_original", 622), ("shape_turbulence", 623),
        ("order_splat_original", 624), ("shape_controlled", 625), ("stats", 626),
    )),
)
SCRIPTS += FEATURE_SCRIPTS

BY_NAME = {s.name: s for s in SCRIPTS}


# ---- the two runners -----------------------------------------------------------------------------------------------------------------------------------------------------


def points_of(origins, seed):
    """N_POINTS positions from points_cases' classes (inside, crossing, rim, outside, far, integer, below, large) with non-finite rows, and one attribute per point with
    non-finite values"""
    import points_cases as pc

    rng = np.random.default_rng([seed, 77])
    xyz = pc.make_points(origins, seed, n=N_POINTS).copy()
    rows = rng.choice(N_POINTS, size=12, replace=False)
    xyz[rows[:4], 0] = np.nan
    xyz[rows[4:8], 1] = np.inf
    xyz[rows[8:], 2] = -np.inf
    attr = rng.standard_normal(N_POINTS).astype(F)
    attr[rng.choice(N_POINTS, size=9, replace=False)] = np.array([np.nan, np.inf, -np.inf] * 3, dtype=F)
    return xyz, attr


@functools.lru_cache(maxsize=None)
def initial_state(name):
    s = BY_NAME[name]
    names = PROFILES[s.profile]
    o = np.ascontiguousarray(fc.random_leaves(s.seed), dtype=np.int32)
    st = fc.random_state(s.seed + 1, len(o), names)
    st["vel"] *= F(0.6)
    xyz, attr = points_of(o, s.seed)
    st.update(origins=o, masks=None, xyz=xyz, attr=attr, splat_spec=DEFAULT_SPEC, live=N_POINTS, names=names, timing=s.timing, method=None, control=None, order_key=None)
    # the motion's rows: the points' positions (their non-finite rows with them), velocities from the attribute as World.vel3 forms them, ages in [0, 1)
    st.update(motion_xyz=xyz.copy(), motion_vel=np.stack([attr, F(-0.5) * attr, F(0.25) * attr], axis=1), motion_age=np.random.default_rng([s.seed, 78]).random(N_POINTS).astype(F))
    return st


def _step(world, script, i):
    name, seed = script.steps[i]
    out = OPS[name].fn(world, np.random.default_rng(seed))
    world.after(OPS[name])
    return out


def run_twin(script: Script, upto=None):
    """-> per step (outputs, captured state): every step on a World of its own, opened from the state the step before left, under lookahead = 0 and a filled pool"""
    import hnanosolver_amd as H
    from pool_cases import arena_fill

    state, out = initial_state(script.name), []
    H.set_option("lookahead", "0")
    try:
        for i in range(len(script.steps) if upto is None else upto):
            with arena_fill(TWIN_FILLS[i % 2]):
                w = World(state)
                try:
                    outputs = _step(w, script, i)
                    captured = w.capture()
                    state = w.carry(captured)
                finally:
                    w.close()
            out.append((outputs, captured))
    finally:
        H.set_option("lookahead", None)
    return out


def run_resident(script: Script, mode, upto=None, against=None):
    """ONE World from the first step to the last, options at their defaults but lookahead = mode -> (per step (outputs, captured state, lookahead_counts), difference).
    against: the twin's records; every step is then compared as soon as it has run, the pass ends at the first difference, and the captured states are not kept"""
    import hnanosolver_amd as H

    out, difference = [], None
    H.set_option("lookahead", mode)
    try:
        w = World(initial_state(script.name))
        try:
            for i in range(len(script.steps) if upto is None else upto):
                outputs = _step(w, script, i)
                record = (outputs, w.capture(), w.sim.lookahead_counts())
                if against is not None:
                    difference = step_difference(script, mode, i, against[i], record)
                    record = (outputs, None, record[2])
                out.append(record)
                if difference:
                    break
        finally:
            w.close()
    finally:
        H.set_option("lookahead", None)
    return out, difference


def as_words(v):
    """an output as 32-bit words where it is an array of them (so that NaN payloads and signed zeros count), else as the bytes pool_cases.as_bytes compares"""
    from pool_cases import as_bytes

    b = as_bytes(v)
    return np.frombuffer(b, dtype=np.uint32) if len(b) % 4 == 0 else np.frombuffer(b, dtype=np.uint8)


def step_difference(script: Script, mode, i, t, r):
    """None, or how step i of the resident pass (r) differs from the twin's (t) in anything the step returned or in the downloaded state"""
    for part, a, b in (("returned", r[0], t[0]), ("state", r[1], t[1])):
        where = f"script {script.name}, lookahead = {mode}, step {i} ({script.steps[i][0]}, after {script.steps[i - 1][0] if i else 'the upload'})"
        if a.keys() != b.keys():
            return f"{where}: the {part} names differ: {sorted(a.keys() ^ b.keys())}"
        for k in a:
            x, y = as_words(a[k]), as_words(b[k])
            if x.shape != y.shape:
                return f"{where}: {part} {k} has {x.size} words on the resident sim and {y.size} on the twin"
            d = np.flatnonzero(x != y)
            if len(d):
                return f"{where}: {part} {k} differs in {len(d)} of {x.size} words, first at word {int(d[0])} ({int(x[d[0]]):#x} resident, {int(y[d[0]]):#x} twin)"
    return None


def first_difference(script: Script, mode, twin, resident):
    """None, or the message of the first step at which the resident and the twin differ"""
    for i, (t, r) in enumerate(zip(twin, resident)):
        d = step_difference(script, mode, i, t, r)
        if d:
            return d
    return None


@functools.lru_cache(maxsize=1)
def twin_record(name):
    """the twin's pass of a script: run before any resident pass and shared by the modes (one script's record is kept at a time: it holds every step's full state)"""
    return run_twin(BY_NAME[name])


def compare(script: Script, mode, upto=None):
    """rerun any prefix of a script both ways -> the first difference or None"""
    return run_resident(script, mode, upto, against=run_twin(script, upto))[1]
