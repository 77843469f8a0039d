"""Mixed call sequences on one device-resident sim against a twin with no hidden state (tests/sequence_cases.py states the vocabulary, the two runners and the scripts;
tests/test_sequence_cases.py holds the scripts' coverage conditions without a GPU).

The twin's pass of a script runs first, every step on a sim, an order and a population of its own that are opened from the documented state alone, with lookahead = 0 and
the pool of device memory filled with a non-zero byte. Then ONE sim runs the script from its first step to its last, once with lookahead = auto and once with
lookahead = 1, and after every step everything the step returned and the full downloaded state must be the twin's, byte for byte. Nothing here is a tolerance.

Byte equality with the twin compares the library with itself, so one collision trace and one neighbourhood query of the twin's pass of frame_points are held once to
the numpy mirrors of the per-call tests (test_the_twin_equals_the_mirrors): a twin that is wrong in the way the resident sim is wrong cannot pass."""
import numpy as np
import pytest

import sequence_cases as sq

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_options():
    import hnanosolver_amd as H

    yield
    for k in ("lookahead", "fuse", "arena_fill"):
        H.set_option(k, None)


def steps_of(script, kinds):
    return [i for i, o in enumerate(script.ops) if o.kind in kinds]


MODE_BIT = {"push": (1, 2), "stop": (2,), "kill": (4,)}  # the bits of `hit` a mode alone sets: pushed, put back, killed
SEEN_BITS = {}  # script name -> {(mode, bit): rows}, over the twin's collision traces; filled by check_liveness


def collide_bits(script, out):
    seen = {}
    for i in steps_of(script, ("trace_collide",)):
        mode = sq.COLLIDE_SPECS[script.steps[i][0]][0]
        for bit in MODE_BIT[mode]:
            seen[(mode, bit)] = seen.get((mode, bit), 0) + int(((out[i]["hit"] & bit) != 0).sum())
    return seen


def check_liveness(script, twin):
    """the script did exercise the state it is about -- counted from the twin's recorded outputs, so that a script which never reaches the hidden state cannot pass empty"""
    names = [k for k, _ in script.steps]
    out = [t[0] for t in twin]
    changes = steps_of(script, ("regrid", "emit"))
    if changes:
        moved = [out[i]["leaves"] for i in changes]
        assert any(a != b for a, b in moved), f"{script.name}: no regrid changed the leaf count: {moved}"
    levels = {int(o["solve_levels"][0]) for o in out if "solve_levels" in o}
    if levels and any(script.ops[i].grid and "solve_levels" in out[i] for i in range(len(out))):  # a V-cycle method and a regrid under it
        assert len(levels) >= 2, f"{script.name}: solve_levels was reported for one leaf count only: {levels}"
    selects = steps_of(script, ("select_compact",))
    if selects:
        kept = [(int((out[i]["slot"] >= 0).sum()), len(out[i]["slot"])) for i in selects]
        assert any(0 < k < n for k, n in kept), f"{script.name}: no select both dropped and kept a point: {kept}"
        for i in selects:
            assert out[i]["counts"][0] == int((out[i]["slot"] >= 0).sum())
    births = steps_of(script, ("birth",))
    if births:
        born = [out[i]["counts"][1] - out[i]["live_before"] for i in births]  # (wanted counts the births that found no row too)
        assert any(b >= 1 for b in born), f"{script.name}: no birth bore a point: {born}"
    if "birth_overflow" in names:
        cut = [out[i]["counts"] for i in births if names[i] == "birth_overflow"]
        assert any(wanted > live for live, wanted in cut), f"{script.name}: the births never overflowed the rows: {cut}"
    if any(t[1]["splat_spec"] != sq.DEFAULT_SPEC for t in twin):
        assert "splat_stored" in names
    collides = steps_of(script, ("trace_collide",))
    if collides:
        met = [(int((out[i]["hit"] == 0).sum()), int((out[i]["hit"] != 0).sum())) for i in collides]
        print(f"{script.name}: collision traces, rows (hit == 0, hit != 0) per step: {met}")
        assert any(a > 0 and b > 0 for a, b in met), f"{script.name}: no collision trace both met and missed the collider: {met}"
        SEEN_BITS[script.name] = collide_bits(script, out)
        print(f"{script.name}: rows per (mode, hit bit): {SEEN_BITS[script.name]}")
    kills = [i for i in collides if names[i] == "trace_collide_kill_compact"]
    if kills:
        kept = [(int((out[i]["slot"] >= 0).sum()), len(out[i]["slot"])) for i in kills]
        print(f"{script.name}: kills (kept, rows): {kept}")
        assert any(0 < k < n for k, n in kept), f"{script.name}: no kill both dropped and kept a point: {kept}"
        for i in kills:
            assert out[i]["counts"][0] == int((out[i]["slot"] >= 0).sum()) == int((out[i]["status"] >= 1).sum())
    queries = steps_of(script, ("neighbours",))
    if queries:
        lone = [(int((out[i]["count"] == 0).sum()), int((out[i]["count"] != 0).sum())) for i in queries]
        print(f"{script.name}: neighbourhood queries, rows (count == 0, count != 0) per step: {lone}")
        assert any(a > 0 and b > 0 for a, b in lone), f"{script.name}: no query found both lone points and points with neighbours: {lone}"
    tables = steps_of(script, ("cells",))
    if tables:
        inner = [(int(((out[i]["cell_start"] > 0) & (out[i]["cell_start"] < out[i]["inside"])).sum()), out[i]["inside"]) for i in tables]
        print(f"{script.name}: cell tables (entries strictly between 0 and inside, inside): {inner}")
        assert any(k > 0 for k, _ in inner), f"{script.name}: no cell table holds an entry strictly between 0 and inside: {inner}"
        for i in tables:
            assert int(out[i]["cell_start"][-1]) == out[i]["inside"] and len(out[i]["cell_start"]) == 512 * twin[i][1]["origins"].shape[0] + 1


@pytest.mark.parametrize("mode", ["auto", "1"])
@pytest.mark.parametrize("name", [s.name for s in sq.SCRIPTS])
def test_resident_sim_equals_its_twin(name, mode):
    script = sq.BY_NAME[name]
    twin = sq.twin_record(name)  # (the twin's pass first, recorded once: arena_fill is never on during a resident pass)
    check_liveness(script, twin)
    resident, difference = sq.run_resident(script, mode, against=twin)  # (compared step by step; ends at the first difference)
    assert difference is None, difference + f" -- rerun a prefix with sequence_cases.compare(BY_NAME[{name!r}], {mode!r}, upto=...)"
    assert len(resident) == len(twin) == len(script.steps)
    counts = [r[2] for r in resident]
    print(f"{name} lookahead = {mode}: {len(script.steps)} steps, {twin[-1][1]['origins'].shape[0]} leaves at the end, lookahead_counts {counts[-1]}")
    if mode == "1":
        want = sq.expected_lookahead(script)
        wrong = [i for i in range(len(want)) if counts[i] != want[i]]
        assert not wrong, (f"script {name}, lookahead = 1, step {wrong[0]} ({script.steps[wrong[0]][0]}): lookahead_counts {counts[wrong[0]]}, the table's memo column gives "
                           f"{want[wrong[0]]}")
        if sq.has_two_equal_substeps(script):
            assert counts[-1][0] >= 1 and counts[-1][1] >= 1, counts[-1]
    else:
        assert all(c[0] >= c[1] for c in counts)


def test_every_collision_mode_sets_its_own_bit_somewhere():
    """bit 1 and bit 2 under push, bit 2 under stop, bit 4 under kill, over the twin's passes of the scripts that trace against the collider (counted by check_liveness
    where the comparison above has run; a script it has not seen runs its twin's pass here)"""
    total = {}
    for script in sq.SCRIPTS:
        if steps_of(script, ("trace_collide",)):
            seen = SEEN_BITS.get(script.name)
            if seen is None:
                seen = collide_bits(script, [t[0] for t in sq.twin_record(script.name)])
            for k, v in seen.items():
                total[k] = total.get(k, 0) + v
    print(f"rows per (mode, hit bit) over the suite: {total}")
    assert set(total) == {(m, b) for m, bits in MODE_BIT.items() for b in bits} and all(v > 0 for v in total.values()), total


def test_the_twin_equals_the_mirrors():
    """frame_points' trace_collide_push against points_collide_cases.collide_mirror, and its first neighbours_original against neighbour_cases.restate, each on the state
    the twin captured in front of the step: words for the positions, bytes for status and hit; bytes of count, density and push for the 1,500 points"""
    import neighbour_cases as nc
    import points_collide_cases as cc
    from hnanosolver_amd import _lib, api
    from oracle_lib import OracleGrid, oracle_device

    script = sq.BY_NAME["frame_points"]
    names = [k for k, _ in script.steps]
    twin = sq.twin_record(script.name)
    # the collision trace (the device-semantics build of the oracle: the script's points hold NaN and infinite rows, whose cell is the GPU's conversion's)
    i = names.index("trace_collide_push")
    before, after = twin[i - 1][1], twin[i]
    mode, order, steps, spec = sq.COLLIDE_SPECS[names[i]]
    assert mode == "push" and before["xyz"].shape == (sq.N_POINTS, 3)
    G = OracleGrid(before["origins"], lib=oracle_device())
    inv_dx = float(np.float32(1.0) / np.float32(sq.VS))
    want, status, hit, _ = cc.collide_mirror(G, before["vel"], before["collision_sdf"], before["xyz"], sq.DT, inv_dx, order, steps, mode, threshold=0.0, **spec)
    got = after[1]["xyz"]
    rows = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    finite = np.isfinite(before["xyz"]).all(1)
    print(f"frame_points step {i}: {len(rows)} rows differ from the mirror in their words, {int(finite[rows].sum())} of them with a finite start; hit bits of the mirror: "
          f"pushed {int((hit & 1 != 0).sum())}, put back {int((hit & 2 != 0).sum())}, none {int((hit == 0).sum())}; moved {int((got.view(np.uint32) != before['xyz'].view(np.uint32)).any(1).sum())}")
    assert (hit & 1 != 0).any() and (hit == 0).any() and (got != before["xyz"]).any(), "the step's points never meet the collider, or all do: the comparison would show little"
    assert np.array_equal(after[0]["status"], status), f"status differs at rows {np.flatnonzero(after[0]['status'] != status)[:8].tolist()}"
    assert np.array_equal(after[0]["hit"], hit), f"hit differs at rows {np.flatnonzero(after[0]['hit'] != hit)[:8].tolist()}"
    assert len(rows) == 0, f"positions differ in rows {rows[:8].tolist()}: {got[rows[:4]].tolist()} against {want[rows[:4]].tolist()}"
    # the neighbourhood query
    j = names.index("neighbours_original")
    before, after = twin[j - 1][1], twin[j][0]
    assert names[j - 1] == "sort_voxel" and np.array_equal(before["origins"], twin[j][1]["origins"])
    grid = api.create_grid_from_leaves(before["origins"], sq.VS, _lib.HNS_GRID_HOST_ONLY)
    r = nc.restate(grid, len(before["origins"]), before["xyz"], 2.0)
    print(f"frame_points step {j}: {int((r.count != 0).sum())} of {len(r.count)} points have neighbours, {len(r.pairs)} pairs, {int(nc.takes_part(grid, len(before['origins']), before['xyz']).sum())} take part")
    assert len(r.count) == sq.N_POINTS and (r.count != 0).any() and (r.count == 0).any() and np.count_nonzero(r.push)
    nc.same((after["count"], after["density"], after["push"]), r, "frame_points' first neighbours_original against the restatement")


def test_the_twin_is_deterministic():
    """two twin passes of a script give the same bytes: the comparison above is of the library, not of the harness"""
    script = sq.BY_NAME["frame_vcycle"]
    a, b = sq.twin_record(script.name), sq.run_twin(script)
    assert sq.first_difference(script, "twin", a, [(o, s, None) for o, s in b]) is None
