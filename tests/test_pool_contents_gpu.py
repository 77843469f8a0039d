"""No result may depend on what pooled device memory held. Almost every byte of device memory the library uses comes from the process-wide pool of hns_arena.hip, and a
block from it holds whatever its previous owner left there; the code relies on "written before it is read" for each of them (make_sim's uncleared sims and its clear list
for an active prefix, the regrid's scratch and the new arena it carries the fields into, the 65-ints-per-block table of hns_sorblock.hip, the grid tables, masks, the
deactivation table, the diagnostics' partial records). GPU tests run in fresh processes, where the driver mostly hands out zero pages and the pool's used blocks hold
ordinary finite field values, so a violation would not show. Option arena_fill (tests/pool_cases.py) makes every block arrive filled with 0x00, 0xFF or 0x7F.

Every test asserts (a) under EACH fill the bits of the independent reference the project already uses for that path -- the oracle, frame_cases.host_chain,
leafio.leaf_stats, diag_cases.residual_numpy, the plain solve of the same iteration count, the single grid -- and (b) that outputs without such a reference (pressure bits,
solve reports, counts, masks, an active prefix's results) are the same bytes under the three fills. Only what the ABI documents as defined is compared: results inside the
launch range, pressure behind a solve. The fill is a device-wide wait, so no call here is captured."""
import functools

import numpy as np
import pytest
import torch

import diag_cases as dc
import hnanosolver_amd as H
import special_cases as sc
from dist_cases import check, partitioned_sim_substeps_match_single_grid, run_local, single_grid
from frame_cases import COMBUST, download, frame_chain, make_sim, make_sources, random_leaves, random_masks, random_state, sdf_source
from grid_cases import assert_device_tables_match_host_builder
from hnanosolver_amd import api, device as D, fields, leafio
from operator_cases import build_data, field_data, snapshot
from oracle_lib import OracleGrid
from pool_cases import FILLS, arena_fill, under_every_fill
from sor_cases import range_sweep

pytestmark = pytest.mark.gpu

OPTIONS = ("arena_fill", "cook_cache", "fuse", "sor_block_lb", "rbgs", "lookahead", "dist_mirror")


@pytest.fixture(autouse=True)
def restore_options():
    yield
    for k in OPTIONS:
        H.set_option(k, None)


def assert_words(got, want, what):
    assert dc.words(got) == dc.words(want), f"{what}: {sc.describe(got, want)}"


def test_the_fill_reaches_the_blocks_and_goes_off_again():
    """The switch itself, without which everything below would pass for nothing. A regrid draws a new arena and writes the velocity and the float fields into it, nothing
    else, so the pressure of a sim that has not solved since is the fill as it arrived. The ABI calls that buffer undefined: it is read here for this purpose alone and
    compared nowhere else (should a regrid ever clear it, this probe has to move to another unwritten buffer)."""
    o = sc.LEAF_SETS["ragged32"]()
    for fill in FILLS:
        with arena_fill(fill):
            seen = set()
            for _ in range(2):  # a block fresh from the driver, then one back from the pool
                g, s = make_sim(o, ["density"], random_state(1, len(o), ["density"]), None, 0.1)
                s.regrid(0)
                seen |= set(np.unique(dc.pressure_of(s).view(np.uint8)).tolist())
                s.close()
            assert seen == {fill}, (fill, seen)
        assert H.get_option("arena_fill") == "off"
    with pytest.raises(ZeroDivisionError):
        with arena_fill(0x7F):
            1 / 0
    assert H.get_option("arena_fill") == "off"


def test_a_new_sim_reads_back_zeros():
    """hns_sim_create clears the fields of the sim it makes: one that was never uploaded to downloads as +0.0 in every field, whatever the block held"""
    o = sc.LEAF_SETS["ragged32"]()
    names = COMBUST + ["collision_sdf"]

    def scenario():
        grid = api.create_grid_from_leaves(o, 0.1)
        s = D.Sim(grid, names)
        got = download(s, names)
        s.close()
        for k, v in got.items():
            assert not v.view(np.uint32).any(), f"{k}: a new sim's field is not +0.0 everywhere"
        return got

    under_every_fill(scenario)


# ---------------------------------------------------------------------------------------------------------------
# 1. the six operators on uncleared memory
# ---------------------------------------------------------------------------------------------------------------

OPERATOR_SETS = {"plume8": (lambda: fields.plume_leaves(8, 1.0, 0.3), 64), "dense16": (lambda: fields.dense_leaves(16), 16)}
DT, SIM_ITERS = 1.0 / 24.0, 6
COMPUTE_CASES = [(coll, fs) for coll in (False, True) for fs in (0.0, 1.0)]


@functools.lru_cache(maxsize=None)
def operator_references(set_name):
    """the oracle's results of every operator call below on the whole grid, computed once"""
    mk, R = OPERATOR_SETS[set_name]
    origins = mk()
    G, vs = OracleGrid(origins), 1.0 / R
    ref = {}
    for coll, fs in COMPUTE_CASES:
        want = snapshot(build_data(origins, R, with_sdf=coll))
        names = [n for n in want if n != "vel"]
        assert G.compute_sim(want["vel"], {n: want[n] for n in names}, SIM_ITERS, DT, vs, api.CombustionParams(factorScale=fs), coll) == 0
        if coll:
            want["collision_sdf"][:] = 0.0  # the reference hands the SDF back zeroed (HNanoSolver.cu:364-369)
        ref["sim", coll, fs] = want
    f = fields.synthetic_fields(origins, R)
    adv = [f["density"].copy(), f["temperature"].copy()]
    G.advect_index_grid(f["vel"], adv, DT, vs)
    ref["advect"] = {"density": adv[0], "temperature": adv[1], "vel": f["vel"]}
    wv = f["vel"].copy()
    G.advect_index_grid_velocity(wv, DT, vs)
    ref["advect_velocity"] = {"vel": wv}
    wp = f["vel"].copy()
    assert G.project_non_divergent(wp, 5, vs) == 0
    ref["project"] = {"vel": wp}
    wd = np.zeros(len(origins) * 512, np.float32)
    G.divergence_op(f["vel"], wd, vs)
    ref["divergence"] = {"divergence": wd, "vel": f["vel"]}
    return ref


def operators_scenario(set_name, cook_cache, prefix):
    """every operator on a new grid; with the cook cache two cooks each, so that the second borrows the sim the first left with the grid. prefix: only the first half of the
    leaves is active (hns_grid_set_active_leaves) -- no oracle for that, the active leaves' results go to the comparison across fills. A prefix's first cook runs on a
    new sim that sim_create cleared, its second on the cached sim behind make_sim's hand-written clear list, with the same inputs: the two must agree"""
    mk, R = OPERATOR_SETS[set_name]
    origins = mk()
    vs, n = 1.0 / R, len(origins)
    n_active = max(1, n // 2) if prefix else n
    ref = None if prefix else operator_references(set_name)
    f = fields.synthetic_fields(origins, R)
    cooks = 2 if cook_cache else 1
    out = {}

    def grid_for(d):
        h = api.IndexGridHandle()
        api.CreateIndexGrid(d, h, vs)
        if prefix:
            h.set_active_leaves(n_active)
        return h

    def record(key, d, want):
        for name, v in snapshot(d).items():
            if want is not None:
                assert_words(v, want[name], f"{set_name} {key} {name}")
            out[f"{key}/{name}"] = v[: n_active * 512]

    H.set_option("cook_cache", str(cook_cache))
    for coll, fs in COMPUTE_CASES:
        for fuse in (1, 0):
            H.set_option("fuse", str(fuse))
            h = grid_for(build_data(origins, R, with_sdf=coll))
            for cook in range(cooks):
                d = build_data(origins, R, with_sdf=coll)
                api.Compute_Sim(d, h, SIM_ITERS, DT, vs, api.CombustionParams(factorScale=fs), coll)
                record(f"sim/coll{int(coll)}/fs{fs}/fuse{fuse}/cook{cook}", d, ref and ref["sim", coll, fs])
            h.reset()
    H.set_option("fuse", None)
    calls = {
        "advect": (("density", "temperature"), lambda d, h: api.AdvectIndexGrid(d, DT, vs, handle=h)),
        "advect_velocity": ((), lambda d, h: api.AdvectIndexGridVelocity(d, DT, vs, handle=h)),
        "project": ((), lambda d, h: api.ProjectNonDivergent(d, 5, vs, handle=h)),
        "divergence": (("divergence",), lambda d, h: api.Divergence(d, vs, handle=h)),
    }
    for key, (floats, call) in calls.items():
        h = grid_for(field_data(origins, f, floats))
        for cook in range(cooks):
            d = field_data(origins, f, floats)
            call(d, h)
            record(f"{key}/cook{cook}", d, ref and ref[key])
        h.reset()
    if prefix:
        for k in [k for k in out if "/cook1/" in k]:
            assert_words(out[k], out[k.replace("/cook1/", "/cook0/")], f"{set_name} {k}: the cached sim behind the clear list against the cleared new sim")
    return out


@pytest.mark.parametrize("prefix", [False, True], ids=["allactive", "prefix"])
@pytest.mark.parametrize("cook_cache", [0, 1])
@pytest.mark.parametrize("set_name", list(OPERATOR_SETS))
def test_operators_on_uncleared_memory(set_name, cook_cache, prefix):
    under_every_fill(lambda: operators_scenario(set_name, cook_cache, prefix))


# ---------------------------------------------------------------------------------------------------------------
# 2. grid and SOR tables
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["ragged32", "sparse_far", "one_leaf"])
def test_grid_tables(name):
    origins = sc.LEAF_SETS[name]()
    under_every_fill(lambda: assert_device_tables_match_host_builder(origins))


SOR_SETS = {"ragged32": sc.LEAF_SETS["ragged32"], "dense16": lambda: fields.dense_leaves(16)}
SOR_DX, SOR_OMEGA = 0.013, 1.93


@functools.lru_cache(maxsize=None)
def sor_case(name):
    """div, p0 and the oracle's sweeps of them, computed once"""
    origins = SOR_SETS[name]()
    rng = np.random.default_rng(3)
    n = len(origins) * 512
    div, p0 = rng.standard_normal(n).astype(np.float32), (rng.random(n) * 2 - 1).astype(np.float32)
    G = OracleGrid(origins)
    return origins, div, p0, {iters: G.rbgs_iterations(div, SOR_DX, SOR_OMEGA, iters, p0) for iters in (1, 2, 3, 7)}


def sor_scenario(name, lb):
    """every iteration count on the whole grid against the oracle, then on a launch range, then on the whole grid again (the SOR tables are drawn anew each time). On a
    range only ONE blocked launch -- two iterations -- equals the oracle's sweeps of the whole grid, because the leaves outside the range are not swept between launches
    (tests/test_sorblock_gpu.py); the other counts have no reference there and go to the comparison across fills"""
    origins, div_h, p0_h, want = sor_case(name)
    n_leaves = len(origins)
    first, count = min(5, n_leaves - 1), min(17, n_leaves - min(5, n_leaves - 1))  # (5, 17); what is left of it on eight leaves
    H.set_option("sor_block_lb", str(lb))
    grid = api.create_grid_from_leaves(origins, SOR_DX)
    div, p0 = torch.from_numpy(div_h).cuda(), torch.from_numpy(p0_h).cuda()
    out = {}

    def sweep(iters):
        p_a, p_b = p0.clone(), torch.full_like(p0, 7.0)  # stale content of the second buffer must not matter
        return D.rbgs_iterate(grid, div, p_a, p_b, SOR_DX, SOR_OMEGA, iters).cpu().numpy()

    for visit in ("whole", "whole_again"):
        for iters in (1, 2, 3, 7):
            got = sweep(iters)
            assert_words(got, want[iters], f"{name} lb={lb} x{iters} {visit}")
            out[f"{visit}/x{iters}"] = got
        if visit == "whole":  # a launch range: two iterations in one launch, the leaves of the range stored, every leaf of the grid a tile source
            grid.set_active_range(first, count)
            for iters in (1, 2, 3, 7):
                got, _, _, sl = range_sweep(grid, div, p0, iters, first, count, SOR_DX, SOR_OMEGA, f"{name} lb={lb} range [{first}, +{count}) x{iters}")
                out[f"range/x{iters}"] = got[sl].cpu().numpy()
            assert_words(out["range/x2"], want[2][sl], f"{name} lb={lb} range [{first}, +{count})")
            grid.set_active_range(0, n_leaves)
    grid.reset()
    return out


@pytest.mark.parametrize("lb", [0, 1, 2])
@pytest.mark.parametrize("name", list(SOR_SETS))
def test_sor_tables(name, lb):
    under_every_fill(lambda: sor_scenario(name, lb))


# ---------------------------------------------------------------------------------------------------------------
# 3. the frame loop of a device-resident sim
# ---------------------------------------------------------------------------------------------------------------

NAMES = COMBUST + ["collision_sdf"]
VS = 1.0 / 32
TOLERANCES, VTOL = {"density": 0.25}, 0.25


def frame_start():
    o = random_leaves(7, n=30)
    return o, random_masks(8, len(o)), random_state(9, len(o), NAMES)


def frame_inputs(frame, origins):
    """a frame's regrid: padding 1 and 9 in turn, an SDF on odd frames, sources of every kind inside and outside the domain"""
    return (9 if frame % 2 else 1), (sdf_source(20 + frame, origins) if frame % 2 else None), make_sources(30 + frame, origins, "mixed", "straddling")


def frame_step(sim, frame):
    sim.substep(4, DT, VS, api.CombustionParams(), frame >= 4)  # (the last two frames with the collision field)


def frames_scenario(lookahead):
    H.set_option("lookahead", lookahead)
    o, m, st = frame_start()
    g, s = make_sim(o, NAMES, st, m, VS)
    frames = frame_chain(s, NAMES, (o, m, st), 6, frame_inputs, frame_step, TOLERANCES, VTOL, VS, keep=[g],
                         probe=lambda sim: (dc.pressure_of(sim), sim.lookahead_counts()))
    counts = [len(o)] + [len(fr[0]) for fr in frames]
    assert any(b < a for a, b in zip(counts, counts[1:])), f"no regrid shrank the domain: {counts}"
    assert any(b > 2 * a for a, b in zip(counts, counts[1:])), f"no regrid outgrew the previous arena: {counts}"
    out = {}
    for i, (origins, regrid_masks, masks, deactivated, got, (pressure, ahead)) in enumerate(frames):
        out.update({f"frame{i}/origins": origins, f"frame{i}/regrid_masks": regrid_masks, f"frame{i}/masks": masks, f"frame{i}/deactivated": deactivated,
                    f"frame{i}/pressure": pressure, f"frame{i}/lookahead_counts": ahead})
        out.update({f"frame{i}/{k}": v for k, v in got.items()})
    s.close()
    return out


@pytest.mark.parametrize("lookahead", ["auto", "1"])
def test_frame_loop_of_a_device_resident_sim(lookahead):
    under_every_fill(lambda: frames_scenario(lookahead))


# ---------------------------------------------------------------------------------------------------------------
# 4. diagnostics on re-drawn tables
# ---------------------------------------------------------------------------------------------------------------


def diagnostics_scenario():
    o, m, st = frame_start()
    g, s = make_sim(o, NAMES, st, m, VS)
    grids = [g]
    frame_chain(s, NAMES, (o, m, st), 1, frame_inputs, frame_step, TOLERANCES, VTOL, VS, keep=grids)
    s.stats(NAMES, velocity=True)  # the diagnostics table exists, at the small leaf count
    before = s.grid.leaf_count()
    grids.append(s.regrid(*frame_inputs(1, s.grid.coords()[::512])))
    origins = s.grid.coords()[::512]
    assert len(origins) > 2 * before, (before, len(origins))
    out = {}
    for masked in (True, False):
        out[f"stats/masked{int(masked)}"] = dc.assert_stats(s, NAMES, masked, f"after a growing regrid, masks {masked}")
    frame_step(s, 1)  # (a substep leaves a divergence for the solves below)
    s.pressure_solve(7, VS)
    div = dc.read_field(dc.lib.hns_sim_divergence_ptr(s._ptr), len(origins))
    p = dc.pressure_of(s)
    rec = s.residual(VS)
    assert rec.tobytes() == leafio.leaf_stats(dc.residual_numpy(origins, div, p, VS)).tobytes(), f"residual after pressure_solve(7): {rec}"
    out["residual"], out["pressure7"] = rec, p
    # the controlled solve against plain solves on a second sim of the same grid
    state = download(s, NAMES)
    g2, b = make_sim(origins, NAMES, state, None, VS)
    dc.set_divergence(b, div)
    rep, stop, plain, initial = dc.controlled_solve_against_plain_solves(s, b, origins, div, VS, 40)
    out.update({"report": (rep["iterations"], rep["checks"], rep["converged"]), "initial": rep["initial"], "final": rep["final"], "history": rep["history"],
                "pressure_controlled": dc.pressure_of(s)})
    s.close(), b.close()
    # caller memory, a launch range on the grid: the statistics cover all leaves, the residual those of the range
    ro = sc.LEAF_SETS["ragged32"]()
    grid = api.create_grid_from_leaves(ro, dc.DX)
    rng = np.random.default_rng(13)
    rdiv, rp = (torch.from_numpy(rng.standard_normal(len(ro) * 512).astype(np.float32)).cuda() for _ in range(2))
    vel, masks = rng.standard_normal((len(ro) * 512, 3)).astype(np.float32), random_masks(6, len(ro))
    grid.set_active_range(5, 17)
    out["range_residual"] = dc.check_residual(grid, ro, rdiv, rp, 5, 17, "range 5+17")
    for values in (rdiv.cpu().numpy(), vel):
        for mk in (None, masks):
            got = D.read_stats(D.field_stats(grid, torch.from_numpy(values).cuda(), None if mk is None else torch.from_numpy(mk).cuda()))
            assert got.tobytes() == leafio.leaf_stats(values, mk).tobytes()
            out[f"field_stats/{values.ndim}/{mk is not None}"] = got
    grid.set_active_range(0, len(ro))
    out["whole_residual"] = dc.check_residual(grid, ro, rdiv, rp, 0, len(ro), "whole grid again")
    grid.reset()
    return out


def test_diagnostics_on_redrawn_tables():
    under_every_fill(diagnostics_scenario)


# ---------------------------------------------------------------------------------------------------------------
# 5. one partitioned case: a rank's grids and SOR tables come from the pool
# ---------------------------------------------------------------------------------------------------------------


def rank_outputs(ranks):
    out = {}
    for r, d in enumerate(ranks):
        got = d.download()
        out[f"rank{r}/vel"] = got["vel"]
        out.update({f"rank{r}/scalar{i}": a for i, a in enumerate(got["scalars"])})
    return out


def partitioned_scenario(path, full):
    """exchanged: the ranks of a few leaves that plume_leaves(8, 1.0, 0.3) gives three ranks. chained: every kernel writes its peers' ghost voxels itself, which the library does
    for ranks swept in 16^3 blocks with sweeps_per_exchange = 2 only -- more than 600 leaves each (hns_dist.hpp: blocked_mirror_rule), so the smallest box that gives three such
    ranks, 13^3 leaves"""
    world = 3
    if path == "exchanged":
        origins, R, k = fields.plume_leaves(8, 1.0, 0.3), 64, 4
        H.set_option("dist_mirror", "0")
    else:
        origins, R, k = fields.dense_leaves(104), 104, 2
    if full:
        params = api.CombustionParams(factorScale=1.0, vorticityScale=0.01, buoyancyStrength=0.05)
        ranks, _ = partitioned_sim_substeps_match_single_grid(origins, R, world, k, 5, 2, params, False)
    else:
        names = ["density", "temperature"]
        _, want = single_grid(origins, R, names, 5, 2)
        ranks = run_local(origins, R, world, k, names, 5, 2)
        check(ranks, want, names)
    assert all(bool(d.info()["chained"]) == (path == "chained") for d in ranks), [d.info()["chained"] for d in ranks]
    return rank_outputs(ranks)


@pytest.mark.parametrize("full", [False, True], ids=["core_substep", "substep"])
@pytest.mark.parametrize("path", ["exchanged", "chained"])
def test_partitioned_substep(path, full):
    under_every_fill(lambda: partitioned_scenario(path, full))
