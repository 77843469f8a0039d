"""The V-cycle pressure solve of a device-resident sim (include/hns.h: "A second solve method") against its numpy mirror tests/mg_cases.py, in every word: the pressure
after 1, 2 and 3 cycles on every leaf set and variant, through both substeps, under a solve control, after a regrid, late on a non-blocking stream -- and the default
path, which must stay the SOR loop. Every test needs hns_sim_set_solve_method, which the code before this feature does not export."""
import functools

import numpy as np
import pytest
import torch

import diag_cases as dc
import hnanosolver_amd as H
import mg_cases as mg
import special_cases as sc
import stream_cases as stc
from frame_cases import COMBUST, assert_same, download, make_sim
from hnanosolver_amd import _lib, api, device as D, leafio
from oracle_lib import OracleGrid, oracle

pytestmark = pytest.mark.gpu

F = np.float32
DX = mg.DX
SETS = {**{k: mg.LEAF_SETS[k] for k in ("one_leaf", "ragged32", "ragged32_off_origin", "sparse_far", "dense32", "ragged_deep")}, "big_ragged": mg.big_ragged}


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in ("sor_block_lb", "rbgs", "lookahead", "arena_fill"):
        H.set_option(k, None)


def assert_words(got, want, what):
    assert dc.words(got) == dc.words(want), f"{what}: {sc.describe(got, want)}"


@functools.lru_cache(maxsize=None)
def case(name):
    o = np.ascontiguousarray(SETS[name](), dtype=np.int32)
    return o, mg.divergence_for(o)


@functools.lru_cache(maxsize=None)
def mirror_solution(name, pre, post, coarse, max_levels, omega):
    """p after each of three cycles, and the leaves per level: computed once per (set, variant), shared and never written"""
    o, div = case(name)
    m = mg.Mirror(o, pre, post, coarse, max_levels, omega)
    ps = m.solve(div, DX, 3, each=True)
    for p in ps:
        p.setflags(write=False)
    return ps, m.leaves_per_level()


def solve_sim(name, names=("density",)):
    o, div = case(name)
    st = {"vel": np.zeros((len(o) * 512, 3), F), **{k: np.zeros(len(o) * 512, F) for k in names}}
    g, s = make_sim(o, list(names), st, None, DX)
    dc.set_divergence(s, div)
    return o, div, s


def check_cycles(name, lb, pre=2, post=2, coarse=8, max_levels=0, omega=1.0):
    o, div, s = solve_sim(name)
    H.set_option("sor_block_lb", lb)
    want, leaves = mirror_solution(name, pre, post, coarse, max_levels, omega)
    s.solve_method(1, pre, post, coarse, max_levels, omega)
    assert s.solve_levels() == leaves
    for cycles in (1, 2, 3):
        s.pressure_solve(cycles, DX)
        assert_words(dc.pressure_of(s), want[cycles - 1], f"{name} lb {lb} V({pre},{post}) coarse {coarse} levels {max_levels} omega {omega}: p after {cycles} cycles")
    # hns_sim_residual works after a V-cycle solve
    assert s.residual(DX)[0].tobytes() == leafio.leaf_stats(dc.residual_numpy(o, div, want[2], DX))[0].tobytes()
    s.close()


@pytest.mark.parametrize("lb", [1, 2])
@pytest.mark.parametrize("name", [k for k in SETS if k != "big_ragged"])
def test_pressure_equals_the_mirror(name, lb):
    check_cycles(name, lb)


def test_pressure_equals_the_mirror_where_the_fine_kernel_is_chosen_by_size():
    """above 600 leaves the 16^3-block SOR kernel runs by itself (sor_block_lb = 0)"""
    o, _ = case("big_ragged")
    assert len(o) > 600
    check_cycles("big_ragged", None)


@pytest.mark.parametrize("variant", [dict(pre=1, post=1), dict(pre=0, post=2), dict(max_levels=2), dict(omega=1.15), dict(pre=1, post=1, omega=1.15, coarse=3)],
                         ids=["V11", "V02", "two_levels", "omega1.15", "V11_omega1.15_coarse3"])
@pytest.mark.parametrize("name,lb", [("ragged32", 1), ("ragged_deep", 2), ("dense32", 2)])
def test_variants_equal_the_mirror(name, lb, variant):
    check_cycles(name, lb, **variant)


# ---------------------------------------------------------------------------------------------------------------
# through the whole substep
# ---------------------------------------------------------------------------------------------------------------

R, DT = 32, 1.0 / 24.0


@functools.lru_cache(maxsize=None)
def substep_state():
    o = np.ascontiguousarray(sc.LEAF_SETS["ragged32"](), dtype=np.int32)
    f = stc.noisy_fields(o, R, 96.0, 4)  # (no signed zeros: the advection kernels match the oracle bit for bit)
    return o, {k: f[k] for k in ["vel"] + COMBUST}


@pytest.mark.parametrize("full", [False, True], ids=["core_substep", "substep"])
def test_substeps_equal_the_mirror_chain(full):
    """the oracle's kernels around the solve, the mirror's V-cycles as the solve: every field, the velocity after the gradient subtraction included, the pressure and
    the divergence. The chain itself is first held against the default method with the oracle's SOR as the solve, so that a difference below is the V-cycle's."""
    o, state = substep_state()
    vs, dt = 1.0 / R, float(F(DT))
    params = api.CombustionParams(factorScale=1.0) if full else None
    G = OracleGrid(o)

    def run(sim, iterations):
        if full:
            sim.substep(iterations, dt, vs, params)
        else:
            sim.core_substep(iterations, dt, vs)
        return download(sim, COMBUST), dc.pressure_of(sim)

    g, s = make_sim(o, COMBUST, state, None, vs)
    got, p = run(s, 6)
    plan_sor = s.substep_plan(params)  # (after the substep, as below: the look-ahead's word depends on the call before)
    omega = float(oracle().orc_omega_compute(vs))
    want, want_p, _ = mg.substep_chain(o, state, COMBUST, dt, vs, lambda div: G.rbgs_iterations(div, float(F(vs)), omega, 6), params)
    assert_same(got, want, "default method against the chain")
    assert_words(p, want_p, "default method: pressure")
    s.close()

    g, s = make_sim(o, COMBUST, state, None, vs)
    s.solve_method()
    m = mg.Mirror(o)
    got, p = run(s, 2)
    want, want_p, want_div = mg.substep_chain(o, state, COMBUST, dt, vs, lambda div: m.solve(div, vs, 2), params)
    assert_words(p, want_p, "V-cycle: pressure")
    assert_same(got, want, "V-cycle against the mirror chain")
    plan = s.substep_plan(params)
    assert plan["pressure"].startswith(f"vcycle<2,2,8>/L{len(m.levels)}:k_rbgs_block") and plan["pressure"].endswith("+k_mg_restrict+k_mg_color+k_mg_prolong")
    assert {k: v for k, v in plan.items() if k != "pressure"} == {k: v for k, v in plan_sor.items() if k != "pressure"}
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# under a control; the default path; refusals
# ---------------------------------------------------------------------------------------------------------------


def test_under_a_control_cycles_are_counted():
    """the loop stops at the first check that meets the bound, p equals the uncontrolled solve of that many cycles, the report and the timing count cycles"""
    name, rel = "ragged_deep", 2e-2
    o, div, a = solve_sim(name)
    _, _, b = solve_sim(name)
    a.solve_method(), b.solve_method()
    initial = leafio.leaf_stats(dc.residual_numpy(o, div, np.zeros_like(div), DX))[0]
    a.solve_control(rel, 0.0, 1)
    a.timing(2)
    a.pressure_solve(12, DX)
    rep = a.solve_report()
    assert rep["initial"].tobytes() == initial.tobytes()
    plain, stop = [], None
    for cycles in range(1, 13):
        b.pressure_solve(cycles, DX)
        plain.append(b.residual(DX)[0])
        if dc.crossed(plain[-1], initial, rel):
            stop = cycles
            break
    print(f"{name}: max|c| at p = 0 {initial['max_abs']:.3e}, per cycle {[float(r['max_abs']) for r in plain]}")
    assert stop is not None and 1 < stop < 12, "the uncontrolled solves do not cross inside the maximum: the case tests nothing"
    assert rep["iterations"] == stop and rep["converged"] and rep["checks"] == stop == len(rep["history"])
    for i, h in enumerate(rep["history"]):
        assert h.tobytes() == plain[i].tobytes(), f"history[{i}]"
    assert_words(dc.pressure_of(a), dc.pressure_of(b), "controlled against uncontrolled")
    assert a.pressure_time()[1] == stop
    # check_every counts cycles too: a check every 2 cycles stops at the first even count that has crossed
    a.solve_control(rel, 0.0, 2)
    a.pressure_solve(12, DX)
    rep2 = a.solve_report()
    assert rep2["iterations"] == stop + (stop & 1) and rep2["checks"] == rep2["iterations"] // 2
    a.close(), b.close()


def test_default_path_and_back_to_sor():
    """a sim that never set a method, one that set and cleared it, and one given method 0 give the same bytes and the same plan as the SOR loop"""
    name = "ragged32"
    o, div, a = solve_sim(name)
    _, _, b = solve_sim(name)
    G = OracleGrid(o)
    omega = float(oracle().orc_omega_compute(DX))
    want = G.rbgs_iterations(div, float(F(DX)), omega, 7)
    plan = a.substep_plan()
    assert plan["pressure"].startswith("k_rbgs_block") and "vcycle" not in plan["pressure"] and "k_mg" not in plan["pressure"]
    a.pressure_solve(7, DX)
    assert_words(dc.pressure_of(a), want, "never set")
    with pytest.raises(RuntimeError):
        a.solve_levels()
    b.solve_method()
    assert b.substep_plan()["pressure"].startswith("vcycle<2,2,8>/L")
    b.pressure_solve(1, DX)
    b.solve_method(None)
    assert b.substep_plan() == plan
    b.pressure_solve(7, DX)
    assert_words(dc.pressure_of(b), want, "set, then cleared")
    b.solve_method(0, pre=-5, omega=9.0)  # (method 0: the other members are not looked at)
    b.pressure_solve(7, DX)
    assert_words(dc.pressure_of(b), want, "method 0")
    a.close(), b.close()


def test_refusals_leave_the_sim_unchanged():
    name = "ragged32"
    o, div, s = solve_sim(name)
    s.solve_method(1, 1, 1, 3, 0, 1.15)
    want = mg.Mirror(o, 1, 1, 3, 0, 1.15).solve(div, DX, 1)
    bad = [dict(method=2), dict(method=-1), dict(pre=-1), dict(post=-1), dict(pre=0, post=0), dict(coarse_iterations=0), dict(max_levels=-1), dict(omega=0.0), dict(omega=2.0),
           dict(omega=-0.5), dict(omega=float("nan")), dict(omega=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            s.solve_method(**kw)
        assert _lib.load_library().hns_last_error()
    s.pressure_solve(1, DX)
    assert_words(dc.pressure_of(s), want, "after the refused setters")
    s.close()


def test_a_capturing_stream_is_refused_only_while_the_hierarchy_is_missing():
    o = np.ascontiguousarray(sc.LEAF_SETS["ragged32"](), dtype=np.int32)
    st = dc.special_state(3, len(o), [])
    st["vel"] = np.random.default_rng(2).standard_normal((len(o) * 512, 3)).astype(F)
    g, s = make_sim(o, [], st, None, DX)
    s.solve_method()
    g2 = s.regrid(1)  # drops the hierarchy
    stream = torch.cuda.Stream()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.stream(stream):
        x.add_(1.0)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            x.add_(1.0)  # (so that the captured graph is not empty; it is never replayed)
            cs = torch.cuda.current_stream().cuda_stream
            for call in (lambda: s.pressure_solve(2, DX, cs), lambda: s.core_substep(2, 0.02, DX, cs)):
                with pytest.raises(ValueError, match="capturing"):
                    call()
    torch.cuda.synchronize()
    assert s.solve_levels()[0] == g2.leaf_count()
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# regrid; late stream
# ---------------------------------------------------------------------------------------------------------------


def test_after_a_regrid_the_new_domain_s_hierarchy_is_used():
    o = np.ascontiguousarray(sc.LEAF_SETS["ragged32"](), dtype=np.int32)
    rng = np.random.default_rng(8)
    st = {"vel": rng.standard_normal((len(o) * 512, 3)).astype(F), "density": rng.standard_normal(len(o) * 512).astype(F)}
    g, s = make_sim(o, ["density"], st, None, DX)
    s.solve_method()
    before = s.solve_levels()
    s.pressure_solve(1, DX)
    g2 = s.regrid(3)  # every voxel is active: the domain grows by the leaves within three voxels
    o2 = g2.coords()[::512].copy()
    assert len(o2) > len(o)
    with pytest.raises(RuntimeError):
        s.residual(DX)  # (no solve on this grid yet)
    div = mg.divergence_for(o2, seed=5)
    dc.set_divergence(s, div)
    s.pressure_solve(2, DX)
    m = mg.Mirror(o2)
    assert_words(dc.pressure_of(s), m.solve(div, DX, 2), "after the regrid")
    assert s.solve_levels() == m.leaves_per_level() and s.solve_levels() != before
    s.close()


def test_late_on_a_non_blocking_stream():
    """a core substep, then the V-cycle solve, on a non-blocking stream on which the sim's state arrives behind a delay: the bytes of the null-stream run"""
    import time

    x = stc.Ctx("scattered")
    delay = stc.Delay(torch)
    names = stc.SIM_NAMES
    state = {k: v for k, v in x.pinned_state().items() if k == "vel" or k in names}
    what = "hns_sim_pressure_solve[vcycle-scattered]"

    def scenario(delay_ms):
        sim = D.Sim(x.grid, names)
        try:
            sim.upload(stc.nan_state(x, names))  # whatever the late upload does not bring is NaN
            sim.solve_method()  # (the setter waits for its own device work: the hierarchy is there before anything is late)
            torch.cuda.synchronize()

            def fn(stream):
                sim.upload(state, stream)
                sim.core_substep(1, x.dt, x.vs, stream)
                sim.pressure_solve(2, x.vs, stream)

            if delay_ms is None:
                t0 = time.perf_counter()
                fn(0)
                host = time.perf_counter() - t0
            else:
                host = None
                stc.late_call(fn, {}, {}, delay, delay_ms, True, None, what)
            return stc.collect_sim(sim, names, True, None), host
        finally:
            torch.cuda.synchronize()
            sim.close()

    want, host = scenario(None)
    assert np.isfinite(want["pressure"]).all() and np.abs(want["pressure"]).max() > 0
    got, _ = scenario(delay.for_host_time(host))
    stc.assert_same_outputs(got, want, f"{what}, late on a non-blocking stream")
