"""The vocabulary and the scripts of tests/test_sequences_gpu.py, checked without a GPU from the declared read / write table and the script lists alone: every entry point
of a sim, a point order, a point population, a point motion, a shaping and a diffusion is an operation or a stated exemption; every pair of operation kinds where the first writes what the second reads is
adjacent in some script; every writer of the velocity and every change of grid sits between two look-ahead substeps; the order's cell table goes through its transitions on
one object; every call that must keep the look-ahead memo sits between two look-ahead substeps too; one Diffusion meets a call with more written fields and a larger grid;
one PointMotion steps either side of a change of grid; no script holds a step the library would refuse. OPS and EXEMPT are whole in tests/sequence_cases.py -- no other module adds to them --, so this file gives the
same answer run alone as in the suite."""
import numpy as np
import pytest

import sequence_cases as sq
from hnanosolver_amd import _lib

PREFIXES = ("hns_sim_", "hns_point_order_", "hns_point_population_", "hns_point_motion_", "hns_shaping_", "hns_diffusion_")
REQUIREMENTS = {"order", "fresh_order", "voxel_order"}


FRAME_POINTS = ["core_substep", "core_substep", "trace_collide_push", "core_substep", "trace_collide_kill_compact", "sort_voxel", "neighbours_original", "neighbours_ranked",
                "order_splat_original", "neighbours_original", "regrid_sdf", "sort_leaf", "sort_voxel", "cell_table", "neighbours_ranked", "substep_collision", "trace_collide_stop"]


def bound_symbols():
    return [n for n in _lib.SIGNATURES if n.startswith(PREFIXES)]


def undecided_symbols(ops):
    used = set(sq.RUNNER_SYMBOLS) | {s for o in ops.values() for s in o.symbols}
    return [n for n in bound_symbols() if n not in used and n not in sq.EXEMPT]


def uncovered_pairs(ops, scripts):
    """the needed pairs of the operations `ops` that no script of `scripts` holds adjacent (a script that names a missing operation holds nothing)"""
    scripts = [s for s in scripts if all(k in ops for k, _ in s.steps)]
    need = {p for p, ways in sq.needed_pairs().items() if any(a in ops and b in ops for a, b in ways)}
    return sorted(need - set(sq.covered_pairs(scripts)))


def test_every_entry_point_is_an_operation_or_exempt():
    """a new hns_sim_* / hns_point_order_* / hns_point_population_* / hns_point_motion_* / hns_shaping_* / hns_diffusion_* entry point fails here until it joins the
    vocabulary or states why it needs no place in it"""
    assert len(bound_symbols()) >= 65  # (50 and the fifteen entry points of the three later prefixes)
    assert {"hns_point_motion_create", "hns_point_motion_destroy", "hns_point_motion_set_stream", "hns_point_motion_get", "hns_shaping_create", "hns_shaping_destroy",
            "hns_shaping_set_stream", "hns_diffusion_create", "hns_diffusion_destroy", "hns_diffusion_set_stream"} <= set(sq.RUNNER_SYMBOLS)
    assert {"hns_point_motion_step", "hns_shaping_apply", "hns_diffusion_apply"} <= {s for o in sq.OPS.values() for s in o.symbols}
    assert not undecided_symbols(sq.OPS), f"entry points that are neither used by an operation of sequence_cases.OPS nor in EXEMPT: {undecided_symbols(sq.OPS)}"
    named = set(sq.RUNNER_SYMBOLS) | set(sq.EXEMPT) | {s for o in sq.OPS.values() for s in o.symbols}
    assert not named - set(_lib.SIGNATURES), f"symbols _lib.py does not bind: {sorted(named - set(_lib.SIGNATURES))}"
    used = set(sq.RUNNER_SYMBOLS) | {s for o in sq.OPS.values() for s in o.symbols}
    assert not used & set(sq.EXEMPT), "an exemption for a symbol that is used"
    assert all(isinstance(r, str) and len(r) > 40 and "\n" not in r for r in sq.EXEMPT.values())


def test_the_table_is_well_formed():
    for name, o in sq.OPS.items():
        assert o.reads <= set(sq.RESOURCES) and o.writes <= set(sq.RESOURCES), name
        assert o.symbols and o.memo in ("produce", "consume", "drop", "keep"), name
        assert o.requires <= REQUIREMENTS and o.sets <= REQUIREMENTS and o.clears <= REQUIREMENTS and not o.sets & o.breaks, name
        assert bool(o.sets) == (o.kind == "sort"), name
        if "order" in o.writes:  # the cell table is a memo of the order: whatever makes another order leaves the table behind
            assert "cells" in o.writes, name
        if "voxel_order" in o.requires:  # (hns_point_order_cells and _neighbours refuse a sort by leaf; Python's xyz must be the positions of that sort)
            assert {"order", "fresh_order"} <= o.requires, name
        assert o.needs <= set(sq.PROFILES["collide"]), name
        if "vel" in o.writes or o.grid:  # include/hns.h: what was looked ahead is dropped by everything else that writes the velocity
            assert o.memo != "keep", name
        if o.memo in ("produce", "consume"):
            assert o.kind in ("substep", "core_substep"), name
    assert len(sq.KINDS) >= 23 and sq.PRODUCERS == {"core_substep", "substep_unfused"}
    assert "cells" in sq.RESOURCES and sq.OPS["sort_voxel"].sets == REQUIREMENTS and sq.OPS["sort_leaf"].breaks == {"voxel_order"}
    assert sq.OPS["regrid_plain"].breaks == REQUIREMENTS and sq.OPS["trace_collide_push"].breaks == {"fresh_order"} and not sq.OPS["gather_scatter"].breaks
    for name in ("trace_collide_stop", "trace_collide_push", "trace_collide_kill_compact"):  # include/hns.h: the sim is only read, and what was looked ahead stays
        o = sq.OPS[name]
        assert o.kind == "trace_collide" and o.memo == "keep" and o.needs == {"collision_sdf"} and "hns_sim_trace_points_collide" in o.symbols, name
        assert {"vel", "grid", "points", "f:collision_sdf"} == o.reads and "points" in o.writes and not o.writes & set(sq.ALL_FIELDS + ("vel", "masks")), name
        assert [p for p in sq.PROFILES if sq.profile_allows(p, o)] == ["collide"], name
    assert "live" in sq.OPS["trace_collide_kill_compact"].writes and "hns_point_population_select" in sq.OPS["trace_collide_kill_compact"].symbols
    for name in ("neighbours_original", "neighbours_ranked", "cell_table"):
        assert sq.OPS[name].requires == REQUIREMENTS and sq.OPS[name].writes == {"cells"} and {"grid", "order", "cells"} <= sq.OPS[name].reads, name
    # include/hns.h: a shape reads no masks; the memo goes with a non-zero amplitude and stays behind a decay alone
    for name, writes, memo in (("shape_turbulence", {"vel"}, "drop"), ("shape_controlled", {"vel", "f:density"}, "drop"), ("shape_decay", {"f:density"}, "keep")):
        o = sq.OPS[name]
        assert o.kind == "shape" and o.writes == writes and o.memo == memo and writes | {"grid"} == o.reads and o.symbols == ("hns_shaping_apply",) and not o.breaks, name
    # a diffuse reads the grid, the masks and what it writes; with collide collision_sdf; the memo goes when the velocity is written
    fields = set(sq.ADVECTED)
    for name, writes, memo, count in (("diffuse_copy", {"f:density"}, "keep", 1), ("diffuse_fields", fields, "keep", 5), ("diffuse_viscosity", {"vel"}, "drop", 0),
                                      ("diffuse_walls", {"vel", "f:density"}, "drop", 1)):
        o = sq.OPS[name]
        collide = sq.DIFFUSE_SPECS[name][4]
        assert o.kind == "diffuse" and o.writes == writes and o.memo == memo and o.reads == writes | {"grid", "masks"} | ({"f:collision_sdf"} if collide else set()), name
        assert len(sq.DIFFUSE_SPECS[name][0]) == count == len(writes - {"vel"}) and ("vel" in writes) == (sq.DIFFUSE_SPECS[name][1] != 0) and not o.breaks, name
        assert all(0.05 <= a <= 4.0 for a in list(sq.DIFFUSE_SPECS[name][0].values()) + [sq.DIFFUSE_SPECS[name][1] or 1.0]), name
        assert ("collision_sdf" in o.needs) == collide and "collision_sdf" not in sq.DIFFUSE_SPECS[name][0], name
    assert sq.DIFFUSE_SPECS["diffuse_copy"][2] == 1 and all(sq.DIFFUSE_SPECS[k][2] >= 2 for k in sq.DIFFUSE_SPECS if k != "diffuse_copy")
    assert {sq.DIFFUSE_SPECS[k][3] for k in sq.DIFFUSE_SPECS} == {"jacobi", "chebyshev"}
    # a motion step only reads the sim and keeps the memo; its object is state of its own, and only a store moves the points
    for name, (mode, steps, spec) in sq.MOTION_SPECS.items():
        o = sq.OPS[name]
        assert o.kind == "motion" and o.memo == "keep" and "motion" in o.writes and {"vel", "grid", "motion"} <= o.reads and "hns_point_motion_step" in o.symbols, name
        assert not o.writes & set(sq.ALL_FIELDS + ("vel", "masks", "points")) and not o.breaks and ("f:collision_sdf" in o.reads) == (mode != "free") == bool(o.needs), name
        if mode != "free":
            assert np.isfinite(spec["max_age"]) and 0 < spec["max_age"] < 1, name  # (the ages are drawn in [0, 1): rows expire)
    assert 0 < sq.MOTION_SPECS["motion_bounce"][2]["restitution"] < 1 and 0 < sq.MOTION_SPECS["motion_bounce"][2]["friction"] < 1
    assert sq.OPS["motion_kill_compact"].writes == {"motion", "live"} and "hns_point_population_select" in sq.OPS["motion_kill_compact"].symbols
    assert sq.OPS["motion_load"].reads == {"points"} and sq.OPS["motion_load"].writes == {"motion"} and sq.OPS["motion_store"].reads == {"motion"}
    assert sq.OPS["motion_store"].writes == {"points"} and sq.OPS["motion_store"].breaks == {"fresh_order"} and "motion" in sq.RESOURCES


def test_every_operation_is_in_a_script_and_every_script_is_of_operations():
    used = {k for s in sq.SCRIPTS for k, _ in s.steps}
    assert not used - set(sq.OPS), f"scripts name operations the vocabulary lacks: {sorted(used - set(sq.OPS))}"
    assert not set(sq.OPS) - used, f"operations no script holds: {sorted(set(sq.OPS) - used)}"
    assert len({s.name for s in sq.SCRIPTS}) == len(sq.SCRIPTS) <= 23  # (a budget of run time: the sixteen of the table before the three features, and their seven)
    assert sq.SCRIPTS[16:] == sq.FEATURE_SCRIPTS and all(len(s.steps) <= 24 for s in sq.FEATURE_SCRIPTS)
    seeds = [sd for s in sq.SCRIPTS for _, sd in s.steps] + [s.seed for s in sq.SCRIPTS]
    assert len(seeds) == len(set(seeds))
    for s in sq.SCRIPTS:
        assert 2 <= len(s.steps) <= 26 and s.profile in sq.PROFILES, s.name
    assert any(s.timing for s in sq.SCRIPTS) and not all(s.timing for s in sq.SCRIPTS)
    assert {s.profile for s in sq.SCRIPTS} == set(sq.PROFILES)
    assert any("birth_overflow" in [k for k, _ in s.steps] for s in sq.SCRIPTS)
    assert [s.name for s in sq.SCRIPTS[:13]] == ["placement_collide", "placement_one", "placement_combust"] + [f"walk_{i}" for i in range(3, 11)] + ["pairs_11", "frame_vcycle"]
    assert sorted(sd for s in sq.SCRIPTS[:13] for sd in [s.seed] + [x for _, x in s.steps]) == list(range(101, 401))  # the regression base keeps its seeds


def test_every_dependent_pair_of_kinds_is_adjacent_in_a_script():
    """(A, B) with A writing what B reads, B followed by the full download both runners take after every step"""
    need = sq.needed_pairs()
    assert len(need) >= 283 and ("splat", "core_substep") in need and ("regrid", "pressure") in need and ("deactivate", "regrid") in need
    assert ("trace", "order_splat") not in need  # (an ordered splat requires a sort since the last write of the positions: never adjacent, by the table's `breaks`)
    for pair in (("sort", "neighbours"), ("neighbours", "neighbours"), ("cells", "neighbours"), ("neighbours", "cells"), ("gather_scatter", "neighbours"), ("trace_collide", "sort"),
                 ("core_substep", "trace_collide"), ("upload", "trace_collide"), ("regrid", "trace_collide"), ("trace_collide", "trace_collide"), ("diffuse", "regrid"),
                 ("deactivate", "diffuse"), ("set_active_masks", "diffuse"), ("diffuse", "substep"), ("shape", "core_substep"), ("regrid", "motion"), ("motion", "motion"),
                 ("motion_store", "sort"), ("motion_store", "trace_collide"), ("motion_load", "motion"), ("diffuse", "motion"), ("shape", "motion"), ("motion", "birth")):
        assert pair in need, pair
    # never adjacent, by `breaks`: the positions moved since the sort; the last sort is by leaf; no order on the new grid
    assert not {("trace_collide", "neighbours"), ("trace", "neighbours"), ("regrid", "neighbours"), ("regrid", "cells"), ("trace_collide", "order_splat"),
                ("motion_store", "neighbours"), ("motion_store", "order_splat")} & set(need)
    assert not [p for p in need if p[0] == "motion" and p[1] not in ("motion", "motion_store", "birth")]  # a motion step writes nothing of the sim
    assert ("sort_leaf", "neighbours_original") not in need[("sort", "neighbours")] and ("sort_leaf", "cell_table") not in need[("sort", "cells")]
    missing = uncovered_pairs(sq.OPS, sq.SCRIPTS)
    assert not missing, f"pairs of operation kinds no script holds adjacent: {missing}"


def runs_of(names, wanted):
    """the positions at which the consecutive steps `names` match `wanted`, a list of sets of operation names"""
    return [i for i in range(len(names) - len(wanted) + 1) if all(names[i + j] in w for j, w in enumerate(wanted))]


def test_the_cell_table_goes_through_its_transitions_in_some_script():
    """what the kinds' pairs alone do not say about the memo of the order object (cell_start behind cells_fresh): each of these is a run of steps on ONE order object
    -- no step of a run changes the grid, by the table's `requires`"""
    query = {"neighbours_original", "neighbours_ranked"}
    runs = {
        "a sort by voxel, by leaf and by voxel again in front of a query": [{"sort_voxel"}, {"sort_leaf"}, {"sort_voxel"}, query],
        "two queries at two radii on one fresh table, the wide group first": [{"neighbours_original"}, {"neighbours_ranked"}],
        "... and the narrow group first, a gather and a scatter between them": [{"neighbours_ranked"}, {"gather_scatter"}, {"neighbours_original"}],
        "a query behind an ordered splat through the same object": [query, {"order_splat_original", "order_splat_ranked"}, query],
        "a query behind a gather and a scatter through the same object": [query, {"gather_scatter"}, query],
        "the table built by its download, then queried": [{"sort_voxel"}, {"cell_table"}, query],
        "the table built by a query, then downloaded twice": [{"sort_voxel"}, query, {"cell_table"}, {"cell_table"}],
        "a query through a new order object behind a regrid": [{"regrid_sdf", "regrid_plain", "regrid_sourced", "regrid_seeded"}, {"sort_leaf"}, {"sort_voxel"}, {"cell_table"}, query],
        "a kill in front of the sort in front of a query": [{"trace_collide_kill_compact"}, {"sort_voxel"}, query],
    }
    for what, wanted in runs.items():
        found = [(s.name, i) for s in sq.SCRIPTS for i in runs_of([k for k, _ in s.steps], wanted)]
        assert found, f"no script holds {what}: {wanted}"
    assert sq.OPS["neighbours_original"].fn is not sq.OPS["neighbours_ranked"].fn


def test_writers_of_the_velocity_sit_between_two_lookahead_substeps():
    """every substep, advect and trace of every script runs with sequence_cases.DT and VS, so two look-ahead substeps either side of a step are substeps of equal dt and
    voxel size: the memo is live when the writer comes"""
    writers = sq.placed_writers()
    assert {"upload_vel", "upload_field", "advect_velocity", "regrid_plain", "regrid_sourced", "regrid_seeded", "regrid_sdf", "emit_trilinear", "emit_radial", "deactivate",
            "splat_velocity", "splat_both", "splat_stored", "order_splat_original", "substep_collision", "substep_fused", "shape_turbulence", "shape_controlled",
            "diffuse_viscosity", "diffuse_walls"} <= set(writers)
    assert "splat_floats" not in writers and "order_splat_ranked" not in writers  # (float fields only: the memo is of the velocity)
    placed = sq.placements(sq.SCRIPTS)
    assert not [k for k in writers if k not in placed], f"never between two look-ahead substeps: {[k for k in writers if k not in placed]}"


KEEPERS = ("shape_decay", "diffuse_copy", "diffuse_fields")


def test_the_calls_that_must_keep_the_memo_sit_between_two_lookahead_substeps():
    """the one prediction a "keep" can fail: with a producer directly on either side, expected_lookahead demands under lookahead = 1 that the substep behind the call
    consumed the memo the substep in front of it left"""
    assert not set(KEEPERS) & set(sq.placed_writers()) and all(sq.OPS[k].memo == "keep" for k in KEEPERS)
    placed = sq.placements(sq.SCRIPTS)
    for k in KEEPERS:
        assert placed.get(k), f"{k} is never directly between two look-ahead substeps"
        name, i = placed[k][0]
        want = sq.expected_lookahead(sq.BY_NAME[name])
        assert want[i] == want[i - 1] and want[i + 1] == (want[i][0] + 1, want[i][1] + 1), (k, name, i)
    for k in ("shape_turbulence", "shape_controlled", "diffuse_viscosity", "diffuse_walls"):  # ... and what a "drop" predicts: nothing is consumed behind it
        name, i = placed[k][0]
        want = sq.expected_lookahead(sq.BY_NAME[name])
        assert want[i + 1] == (want[i][0] + 1, want[i][1]), (k, name, i)


def written_fields(name):
    return len(sq.DIFFUSE_SPECS[name][0])


def test_one_diffusion_meets_more_fields_and_a_larger_grid_in_one_script():
    """the resident World's one Diffusion keeps its pooled block between calls: in ONE script a diffuse with more written float fields comes behind one with fewer (the block
    is carved anew and drawn larger), and a diffuse comes behind a change of grid"""
    found = []
    for s in sq.SCRIPTS:
        names = [k for k, _ in s.steps]
        at = [i for i, k in enumerate(names) if k in sq.DIFFUSE_SPECS]
        more = any(written_fields(names[j]) > written_fields(names[i]) for n, i in enumerate(at) for j in at[n + 1:])
        regridded = any(sq.OPS[names[g]].grid for i in at[:1] for g in range(i + 1, at[-1]))  # a change of grid between the script's first diffuse and its last
        if more and regridded:
            found.append(s.name)
    assert "memo_kept" in found, found
    assert sorted(written_fields(k) for k in sq.DIFFUSE_SPECS) == [0, 1, 1, 5]


def test_one_motion_steps_either_side_of_a_change_of_grid():
    """the PointMotion is documented to survive regrids: in some script a motion step, a change of grid and a motion step, with no motion_load between them (World.after
    drops the order and the population there, and must not drop the motion)"""
    found = []
    for s in sq.SCRIPTS:
        ops = s.ops
        for i, o in enumerate(ops):
            if o.grid and i and ops[i - 1].kind == "motion":
                j = next((j for j in range(i + 1, len(ops)) if ops[j].kind in ("motion", "motion_load")), None)
                if j is not None and ops[j].kind == "motion" and not any(x.grid for x in ops[i + 1:j]):
                    found.append((s.name, i))
    assert ("motion_regrid", 3) in found and ("motion_regrid", 6) in found, found


FRAME_HALF = ["core_substep", "shape_controlled", "diffuse_walls", "core_substep", "motion_load", "motion_bounce", "motion_kill_compact", "motion_store", "sort_voxel",
              "order_splat_original"]


def test_frame_shaped_is_the_frame_loop_on_two_grids():
    s = sq.BY_NAME["frame_shaped"]
    assert [k for k, _ in s.steps] == FRAME_HALF + ["regrid_sdf"] + FRAME_HALF and s.profile == "collide"
    # shape_controlled and diffuse_walls both drop the memo; the motion steps, the sort and the store keep it, the ordered splat of the velocity drops it
    assert sq.expected_lookahead(s)[:11] == [(1, 0), (1, 0), (1, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0)]


def test_no_script_holds_a_step_that_would_be_refused():
    for s in sq.SCRIPTS:
        assert not sq.refusals(s), f"script {s.name}: {sq.refusals(s)}"
    bad = sq.Script("bad", "one", 1, False, (("sort_voxel", 2), ("trace", 3), ("order_splat_original", 4), ("regrid_plain", 5), ("gather_scatter", 6), ("substep_fused", 7)))
    assert [i for i, _ in sq.refusals(bad)] == [2, 4, 5]  # positions moved since the sort; no order on the new grid; a field the profile lacks
    bad = sq.Script("bad", "collide", 1, False, tuple((k, i) for i, k in enumerate(
        ["neighbours_original", "sort_leaf", "cell_table", "sort_voxel", "neighbours_ranked", "trace_collide_stop", "neighbours_ranked", "gather_scatter", "sort_voxel", "sort_leaf",
         "neighbours_original", "sort_voxel", "regrid_sdf", "cell_table"])))
    assert [i for i, _ in sq.refusals(bad)] == [0, 2, 6, 10, 13]  # no sort yet; a sort by leaf; positions moved; by leaf again; no order on the new grid
    assert [i for i, _ in sq.refusals(sq.Script("bad", "combust", 1, False, (("trace_collide_push", 1), ("trace", 2))))] == [0]  # no collision_sdf in the profile


@pytest.mark.parametrize("gone", [("deactivate", "deactivate_counts"), ("pressure_residual",), ("order_splat_original", "order_splat_ranked"), ("birth", "birth_append", "birth_overflow"),
                                  ("trace_collide_stop", "trace_collide_push", "trace_collide_kill_compact"), ("neighbours_original", "neighbours_ranked", "cell_table"),
                                  ("shape_turbulence", "shape_controlled", "shape_decay"), ("diffuse_copy", "diffuse_fields", "diffuse_viscosity", "diffuse_walls"),
                                  ("motion_free", "motion_stick", "motion_bounce", "motion_kill_compact")])
def test_a_deleted_operation_is_noticed(gone):
    """the conditions name what goes uncovered when an operation leaves the vocabulary"""
    ops = {k: o for k, o in sq.OPS.items() if k not in gone}
    lost = {s for k in gone for s in sq.OPS[k].symbols} - set(sq.RUNNER_SYMBOLS) - {s for o in ops.values() for s in o.symbols}
    assert lost and set(undecided_symbols(ops)) == lost
    assert uncovered_pairs(ops, sq.SCRIPTS)  # (the scripts that named it no longer count)


def test_expected_lookahead_counts():
    s = sq.Script("x", "combust", 1, False, tuple((k, i) for i, k in enumerate(
        ["core_substep", "substep_unfused", "splat_floats", "core_substep", "deactivate", "core_substep", "substep_fused", "core_substep", "substep_collision", "core_substep"])))
    #                                 produce  consume+produce  keep    consume+produce  drop    produce  consume  produce  drop    produce
    assert sq.expected_lookahead(s) == [(1, 0), (2, 1), (2, 1), (3, 2), (3, 2), (4, 2), (4, 3), (5, 3), (5, 3), (6, 3)]
    # a collision trace of every mode keeps a live memo, and the substep behind it consumes it: what frame_points opens with
    t = sq.Script("t", "collide", 1, False, tuple((k, i) for i, k in enumerate(
        ["core_substep", "core_substep", "trace_collide_push", "core_substep", "trace_collide_kill_compact", "trace_collide_stop", "core_substep"])))
    assert sq.expected_lookahead(t) == [(1, 0), (2, 1), (2, 1), (3, 2), (3, 2), (3, 2), (4, 3)]
    assert [k for k, _ in sq.BY_NAME["frame_points"].steps] == FRAME_POINTS and sq.BY_NAME["frame_points"].profile == "collide"
    assert sq.expected_lookahead(sq.BY_NAME["frame_points"])[:5] == [(1, 0), (2, 1), (2, 1), (3, 2), (3, 2)]
    assert sq.has_two_equal_substeps(s) and not sq.has_two_equal_substeps(sq.Script("y", "one", 1, False, (("core_substep", 1), ("stats", 2), ("core_substep", 3))))
    assert sum(sq.has_two_equal_substeps(s) for s in sq.SCRIPTS) >= 3


def test_first_difference_names_script_mode_step_operations_array_and_words():
    s = sq.SCRIPTS[0]
    a = np.arange(12, dtype=np.float32)
    twin = [({"status": np.zeros(5, dtype=np.uint8)}, {"vel": a.copy(), "live": None}) for _ in range(3)]
    same = [({"status": np.zeros(5, dtype=np.uint8)}, {"vel": a.copy(), "live": None}, (0, 0)) for _ in range(3)]
    assert sq.first_difference(s, "1", twin, same) is None
    same[2][1]["vel"][7] = -a[7]
    same[2][1]["vel"][9] = np.nan
    msg = sq.first_difference(s, "1", twin, same)
    assert msg.startswith(f"script {s.name}, lookahead = 1, step 2 ({s.steps[2][0]}, after {s.steps[1][0]}): state vel differs in 2 of 12 words, first at word 7"), msg
    same[1][0]["status"][4] = 1  # an earlier step, in what it returned; a byte array compares byte by byte
    assert "step 1" in sq.first_difference(s, "1", twin, same) and "returned status differs in 1 of 5" in sq.first_difference(s, "1", twin, same)
    zero = [({}, {"vel": np.zeros(2, dtype=np.float32)})]
    assert "differs in 1 of 2 words" in sq.first_difference(s, "auto", zero, [({}, {"vel": np.array([0.0, -0.0], dtype=np.float32)}, (0, 0))])  # a zero's sign counts


def test_the_generator_still_draws_scripts_that_meet_the_conditions():
    """the committed lists are what is tested; the generator is kept to draw new ones when the table grows, so it must keep working on the table as it stands"""
    drawn, left = sq.draw_scripts(max_scripts=24)
    assert not left and not uncovered_pairs(sq.OPS, drawn) and len(drawn) <= 20
    assert not [k for k in sq.placed_writers() if k not in sq.placements(drawn)]
    assert all(not sq.refusals(s) and len(s.steps) <= 24 for s in drawn)
    assert "Script(" in sq.format_scripts(drawn)
    placed = sq.placements(drawn)  # (the placement scripts put every writer between two producers; the keepers are placed by hand in memo_kept)
    assert {"shape_turbulence", "shape_controlled", "diffuse_viscosity", "diffuse_walls"} <= set(placed)
    # restricted to the pairs a grown table adds: what FEATURE_SCRIPTS' walks were drawn with
    added = {p for p in sq.needed_pairs() if {"shape", "diffuse", "motion", "motion_load", "motion_store"} & set(p)}
    more, left = sq.draw_scripts(seed=2027, only=added, first_seed=1001, max_scripts=10)
    assert len(added) == 81 and not left and added <= set(sq.covered_pairs(more)) and all(not sq.refusals(s) and len(s.steps) <= 24 for s in more)
    assert min(sd for s in more for _, sd in s.steps) > 1001 and not any(s.name.startswith("placement") for s in more)
