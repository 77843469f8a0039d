"""The diagnostics on the MI355X: Sim.stats against leafio.leaf_stats of the downloaded fields in every byte (ragged and dense, masked or not, after a
deactivation and after a sourced regrid), hns_dev_residual's field against the numpy restatement of c and its record against leaf_stats(c) behind both
SOR kernels and on a launch range, and the controlled solve against plain solves of every multiple of check_every: first crossing, history, same bits."""
import numpy as np
import pytest
import torch

import diag_cases as dc
import hnanosolver_amd as H
import special_cases as sc
from diag_cases import DX, EVERY, REL, assert_stats, check_residual, crossed, host_stats, pressure_of, set_divergence, special_state, words
from frame_cases import COMBUST, assert_same, download, make_sim, make_sources, random_leaves, random_masks
from hnanosolver_amd import _lib, api, device as D, fields, leafio
from hnanosolver_amd._lib import lib

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in ("rbgs", "sor_block_lb", "lookahead"):
        H.set_option(k, None)


# ---------------------------------------------------------------------------------------------------------------
# field statistics
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masks"])
@pytest.mark.parametrize("leaf_set", ["random60", "dense32"])
def test_sim_stats_equal_the_host_mirror(leaf_set, masked):
    names = COMBUST + ["collision_sdf"]
    o = random_leaves(7, n=60) if leaf_set == "random60" else fields.dense_leaves(32)
    st = special_state(8, len(o), names)
    g, s = make_sim(o, names, st, random_masks(9, len(o)) if masked else None)
    got = assert_stats(s, names, masked, "uploaded")
    assert got["nan_count"][-3:].sum() > 0 and np.isinf(got["max_abs"][-3:]).any()  # (the planted velocity: NaN counted, inf a value)
    # one float field alone, the velocity alone, and a sim with masks asked for every voxel
    one = s.stats(["fuel"], masks=masked)
    assert one.tobytes() == got[names.index("fuel"):names.index("fuel") + 1].tobytes()
    assert s.stats([], velocity=True, masks=masked).tobytes() == got[-3:].tobytes()
    if masked:
        assert s.stats(names, velocity=True, masks=False).tobytes() == host_stats(s, names, False)[0].tobytes()
    # after a deactivation the masks are the sim's own
    s.deactivate({"density": 0.5}, 0.5)
    assert_stats(s, names, True, "after deactivate")
    # after a sourced regrid: new leaves, collision_sdf filled with bytes 0x01 (a subnormal) where it had no leaf
    s.regrid(1, None, make_sources(10, o, "mixed", "straddling"))
    got = assert_stats(s, names, True, "after a sourced regrid")
    sdf = download(s, names)["collision_sdf"]
    assert (sdf.view(np.uint32) == 0x01010101).any()
    assert_stats(s, names, False, "after a sourced regrid, every voxel")
    s.close()


def test_sim_stats_refusals_leave_out_untouched():
    o = random_leaves(3, n=10)
    g, s = make_sim(o, ["density", "fuel"], special_state(4, len(o), ["density", "fuel"]))
    for names, velocity in ((["nope"], False), (["density", "density"], False), ([], False)):
        with pytest.raises(ValueError):
            s.stats(names, velocity=velocity)
    arr = (_lib.hns_stats_field * 2)()
    arr[0].name, arr[0].ncomp, arr[1].name, arr[1].ncomp = None, 3, b"v", 3
    out = np.full(6 * leafio.STATS_DTYPE.itemsize, 0x55, dtype=np.uint8)
    before = out.tobytes()
    assert lib.hns_sim_stats(s._ptr, arr, 2, 1, out.ctypes.data, None) == _lib.HNS_ERR_INVALID_ARGUMENT  # two velocity entries
    arr[0].name, arr[0].ncomp = b"density", 3
    assert lib.hns_sim_stats(s._ptr, arr, 1, 1, out.ctypes.data, None) == _lib.HNS_ERR_INVALID_ARGUMENT  # ncomp 3 under a float field's name
    assert lib.hns_sim_stats(s._ptr, None, 1, 1, out.ctypes.data, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert out.tobytes() == before
    with pytest.raises(_lib.HNSError):
        s.residual(DX)  # no solve has run
    s.close()


def test_dev_field_stats_on_caller_memory():
    o = sc.LEAF_SETS["ragged32"]()
    g = api.create_grid_from_leaves(o, DX)
    st = special_state(5, len(o), ["a"])
    m = random_masks(6, len(o))
    for values in (st["a"], st["vel"]):
        for masks in (None, m):
            buf = D.field_stats(g, torch.from_numpy(values).cuda(), None if masks is None else torch.from_numpy(masks).cuda())
            assert D.read_stats(buf).tobytes() == leafio.leaf_stats(values, masks).tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the residual kernel
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("lb", [0, 1, 2])
@pytest.mark.parametrize("leaf_set", ["ragged32", "dense32", "sparse_far", "one_leaf"])
def test_residual_field_and_record_behind_both_sor_kernels(leaf_set, lb):
    o = sc.LEAF_SETS[leaf_set]()
    grid = api.create_grid_from_leaves(o, DX)
    rng = np.random.default_rng(12)
    div = torch.from_numpy(rng.standard_normal(len(o) * 512).astype(F)).cuda()
    H.set_option("sor_block_lb", str(lb))
    for iters in (0, 1, 2, 3, 7):
        p_a, p_b = torch.zeros_like(div), torch.full_like(div, 3.0)
        p = D.rbgs_iterate(grid, div, p_a, p_b, DX, 1.7, iters)
        rec = check_residual(grid, o, div, p, 0, len(o), f"{leaf_set} lb={lb} x{iters}")
        assert rec["count"][0] == len(o) * 512 and rec["nan_count"][0] == 0


@pytest.mark.parametrize("cls", ["nonfinite", "subnormal", "huge", "zeros"])
def test_residual_on_special_values(cls):
    o = sc.LEAF_SETS["ragged32"]()
    grid = api.create_grid_from_leaves(o, DX)
    w = sc.Workload(o, cls, "fields")
    check_residual(grid, o, torch.from_numpy(w.div).cuda(), torch.from_numpy(w.p0).cuda(), 0, len(o), cls)


def test_residual_on_a_launch_range():
    o = sc.LEAF_SETS["ragged32"]()
    grid = api.create_grid_from_leaves(o, DX)
    rng = np.random.default_rng(13)
    div = torch.from_numpy(rng.standard_normal(len(o) * 512).astype(F)).cuda()
    p = torch.from_numpy(rng.standard_normal(len(o) * 512).astype(F)).cuda()
    whole = check_residual(grid, o, div, p, 0, len(o), "whole grid")
    for first, count in ((5, 17), (0, 9), (31, 1)):
        grid.set_active_range(first, count)
        rec = check_residual(grid, o, div, p, first, count, f"range {first}+{count}")
        assert rec["count"][0] == count * 512 and rec.tobytes() != whole.tobytes()
    grid.set_active_range(0, len(o))
    assert check_residual(grid, o, div, p, 0, len(o), "whole grid again").tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the controlled solve
# ---------------------------------------------------------------------------------------------------------------

MAXIT = 100
SETS = {"box16": lambda: fields.dense_leaves(16), "ragged32": sc.LEAF_SETS["ragged32"]}


def solve_sims(leaf_set, names=("density",), seed=20):
    o = np.ascontiguousarray(SETS[leaf_set](), dtype=np.int32)
    rng = np.random.default_rng(seed)
    st = {"vel": rng.standard_normal((len(o) * 512, 3)).astype(F)}
    for k in names:
        st[k] = np.abs(rng.standard_normal(len(o) * 512)).astype(F) * F(0.2)
    div = rng.standard_normal(len(o) * 512).astype(F)
    sims = [make_sim(o, list(names), st, None, DX)[1] for _ in range(2)]
    for s in sims:
        set_divergence(s, div)
    return o, st, div, sims


@pytest.mark.parametrize("leaf_set", list(SETS))
def test_controlled_pressure_solve_stops_at_the_first_crossing(leaf_set):
    o, st, div, (a, b) = solve_sims(leaf_set)
    a.timing(4)
    rep, stop, plain, initial = dc.controlled_solve_against_plain_solves(a, b, o, div, DX, MAXIT)
    print(f"{leaf_set}: first crossing of {REL} at iteration {stop}; max_abs initial {initial['max_abs']:.3e}, history {[float(h['max_abs']) for h in rep['history']]}")
    assert stop is not None, "the plain solves never cross within the maximum"
    assert rep["iterations"] == stop and rep["converged"] and rep["checks"] == stop // EVERY == len(rep["history"])
    ms, iters = a.pressure_time()
    assert iters == stop  # hns_sim_timing counts the iterations that ran
    # control off after on: the parent's bits again
    a.solve_control(None)
    a.pressure_solve(MAXIT, DX)
    b.pressure_solve(MAXIT, DX)
    assert words(pressure_of(a)) == words(pressure_of(b))
    with pytest.raises(_lib.HNSError):
        a.solve_report()
    a.close(), b.close()


@pytest.mark.parametrize("full", [False, True], ids=["core_substep", "substep"])
@pytest.mark.parametrize("leaf_set", list(SETS))
def test_controlled_substeps_equal_the_uncontrolled_run_with_that_many_iterations(leaf_set, full):
    names = COMBUST
    o, st, div, (a, b) = solve_sims(leaf_set, names)
    params = api.CombustionParams()
    dt = 0.02
    a.solve_control(REL, 0.0, EVERY)
    for step in range(2):  # (the second substep consumes the first one's look-ahead on both sims)
        if full:
            a.substep(MAXIT, dt, DX, params)
        else:
            a.core_substep(MAXIT, dt, DX)
        rep = a.solve_report()
        K = rep["iterations"]
        assert K % EVERY == 0 and EVERY <= K <= MAXIT and rep["checks"] == K // EVERY
        assert bool(rep["converged"]) == bool(crossed(rep["final"], rep["initial"]))
        assert not any(crossed(h, rep["initial"]) for h in rep["history"][:-1]), "an earlier check had crossed already"
        if full:
            b.substep(K, dt, DX, params)
        else:
            b.core_substep(K, dt, DX)
        assert_same(download(a, names), download(b, names), f"{leaf_set} step {step}: {K} iterations")
        assert words(pressure_of(a)) == words(pressure_of(b))
        assert b.residual(DX)[0].tobytes() == rep["final"].tobytes()
    assert a.lookahead_counts() == b.lookahead_counts()
    a.close(), b.close()


def test_monitor_only_runs_to_the_maximum():
    o, st, div, (a, b) = solve_sims("box16")
    a.solve_control(0.0, 0.0, EVERY)
    a.pressure_solve(MAXIT, DX)
    rep = a.solve_report()
    assert rep["iterations"] == MAXIT and not rep["converged"] and rep["checks"] == MAXIT // EVERY == len(rep["history"])
    b.pressure_solve(MAXIT, DX)
    assert words(pressure_of(a)) == words(pressure_of(b)) and rep["final"].tobytes() == b.residual(DX)[0].tobytes()
    # a maximum that is no multiple of check_every: the last check is at the maximum
    a.solve_control(0.0, 0.0, 8)
    a.pressure_solve(21, DX)
    rep = a.solve_report()
    assert rep["iterations"] == 21 and rep["checks"] == 3
    b.pressure_solve(21, DX)
    assert words(pressure_of(a)) == words(pressure_of(b))
    a.close(), b.close()


def test_a_planted_nan_runs_to_the_maximum():
    o, st, div, (a, b) = solve_sims("box16")
    div = div.copy()
    div[1234] = np.nan
    set_divergence(a, div)
    a.solve_control(REL, 1e30, EVERY)  # (an absolute tolerance any finite residual meets: only the NaN keeps the loop going)
    a.pressure_solve(20, DX)
    rep = a.solve_report()
    assert rep["iterations"] == 20 and not rep["converged"] and rep["initial"]["nan_count"] == 1 and all(h["nan_count"] > 0 for h in rep["history"])
    a.close(), b.close()


def test_control_refusals_and_a_capturing_stream():
    o, st, div, (a, b) = solve_sims("box16")
    for bad in ((-1.0, 0.0, 4), (float("nan"), 0.0, 4), (0.0, -1e-3, 4), (1e-3, 0.0, 0)):
        with pytest.raises(ValueError):
            a.solve_control(*bad)
    a.solve_control(REL, 0.0, EVERY)
    a.pressure_solve(8, DX)  # (first use of the diagnostics memory, outside the capture)
    before, p_before, rep_before = download(a, ["density"]), pressure_of(a), a.solve_report()
    stream = torch.cuda.Stream()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.stream(stream):
        x.add_(1.0)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            x.add_(1.0)  # (so that the captured graph is not empty; it is never replayed)
            cs = torch.cuda.current_stream().cuda_stream
            for call in (lambda: a.pressure_solve(MAXIT, DX, cs), lambda: a.core_substep(MAXIT, 0.02, DX, cs), lambda: a.substep(MAXIT, 0.02, DX, api.CombustionParams(), False, cs)):
                with pytest.raises(ValueError, match="capturing"):
                    call()
    torch.cuda.synchronize()
    assert_same(download(a, ["density"]), before, "fields after the refused calls")
    assert words(pressure_of(a)) == words(p_before) and a.solve_report()["iterations"] == rep_before["iterations"]
    a.close(), b.close()
