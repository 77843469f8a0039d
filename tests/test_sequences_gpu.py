"""Mixed call sequences on one device-resident sim against a twin with no hidden state (tests/sequence_cases.py states the vocabulary, the two runners and the scripts;
tests/test_sequence_cases.py holds the scripts' coverage conditions without a GPU).

The twin's pass of a script runs first, every step on a sim, an order and a population of its own that are opened from the documented state alone, with lookahead = 0 and
the pool of device memory filled with a non-zero byte. Then ONE sim runs the script from its first step to its last, once with lookahead = auto and once with
lookahead = 1, and after every step everything the step returned and the full downloaded state must be the twin's, byte for byte. Nothing here is a tolerance.

The resident World keeps its PointMotion, its Shaping and its Diffusion through every change of grid (they are bound to no grid); the twin makes them anew for every step.
check_liveness counts, on the twin's record and the state captured in front of each step, what the shape, diffuse and motion steps met -- velocity words moved, the
control below, inside and above its range, inactive and solid voxels, words changed and kept, status 0 and 1, the hit bits, rows expired by age, rows a kill kept --
and prints each count before it asserts.

Byte equality with the twin compares the library with itself, so one collision trace and one neighbourhood query of the twin's pass of frame_points, and one controlled
shape, one diffuse with walls and one bounce of its pass of frame_shaped, are held once to the numpy mirrors of the per-call tests (test_the_twin_equals_the_mirrors):
a twin that is wrong in the way the resident sim is wrong cannot pass."""
import numpy as np
import pytest

import frame_cases as fc
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


HIT_BITS = (1, 2, 4, 8, 16)  # of a motion step: bounced, put back (or stuck), killed, started inside, reflected
FEATURE_SEEN = {}  # script name -> counts over the twin's shape, diffuse and motion steps; filled by check_liveness


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def state_before(script, twin, i):
    """the state the twin's step i was opened from"""
    return twin[i - 1][1] if i else sq.initial_state(script.name)


def active_of(state):
    n = 512 * len(state["origins"])
    return np.ones(n, bool) if state["masks"] is None else fc.unpack(state["masks"]).reshape(-1)


def feature_counts(script, twin):
    """what the twin's shape, diffuse and motion steps of a script met, from its record and the state captured in front of each step; asserts what EVERY such step must
    show and returns the counts that only the suite as a whole must show"""
    names = [k for k, _ in script.steps]
    out = [t[0] for t in twin]
    seen = {}

    def add(key, n):
        seen[key] = seen.get(key, 0) + int(n)

    for i in steps_of(script, ("shape",)):
        before, after = state_before(script, twin, i), twin[i][1]
        moved = int((words(after["vel"]) != words(before["vel"])).sum())
        faded = int((words(after["density"]) != words(before["density"])).sum())
        line = f"{script.name} step {i} ({names[i]}): {moved} velocity words and {faded} density words changed"
        if names[i] == "shape_decay":
            assert moved == 0 and faded > 0, line
        else:
            assert moved > 0 and (faded > 0) == (names[i] == "shape_controlled"), line
        if names[i] == "shape_controlled":
            c, lo, hi = before["density"], np.float32(sq.CONTROL["control_lo"]), np.float32(sq.CONTROL["control_hi"])
            split = (int((c < lo).sum()), int(((c >= lo) & (c <= hi)).sum()), int((c > hi).sum()))
            line += f"; control (below, inside, above): {split}"
            assert all(split), line
        print(line)
    for i in steps_of(script, ("diffuse",)):
        before, after = state_before(script, twin, i), twin[i][1]
        fields, viscosity, _, _, collide = sq.DIFFUSE_SPECS[names[i]]
        written = list(fields) + (["vel"] if viscosity else [])
        changed = sum(int((words(after[k]) != words(before[k])).sum()) for k in written)
        total = sum(words(before[k]).size for k in written)
        active = active_of(before)
        line = f"{script.name} step {i} ({names[i]}): {changed} of {total} words of {written} changed; {int((~active).sum())} of {active.size} voxels inactive"
        add("diffuse steps with inactive voxels", not active.all())
        if collide:
            solid = before["collision_sdf"] < np.float32(0.0)
            line += f", {int(solid.sum())} solid, {int((active & ~solid).sum())} unknowns"
            add("diffuse_walls steps with solid voxels and unknowns", solid.any() and (active & ~solid).any())
        print(line)
        assert 0 < changed < total, line
        for k in after:  # what the call does not list keeps every byte (masks=None in the initial state is every bit set)
            if k not in written and not (k == "masks" and before[k] is None):
                assert np.array_equal(sq.as_words(after[k]), sq.as_words(before[k])), (line, k)
    motions = steps_of(script, ("motion",))
    for i in motions:
        mode, _, spec = sq.MOTION_SPECS[names[i]]
        before, status, hit = state_before(script, twin, i), out[i]["status"], out[i]["hit"]
        for bit in HIT_BITS:
            add((mode, bit), ((hit & bit) != 0).sum())
        age = before["motion_age"].copy()
        for _ in range(out[i]["steps"]):
            age = age + np.float32(sq.DT)
        with np.errstate(invalid="ignore"):  # rows that took their steps, were not killed, and end at or beyond max_age: the mirror of the status rule's last clause
            expired = np.isfinite(before["motion_xyz"]).all(1) & ((hit & 4) == 0) & ~(age < np.float32(spec.get("max_age", np.inf)))
        assert not status[expired].any(), f"{script.name} step {i} ({names[i]}): rows at or beyond max_age with status 1: {np.flatnonzero(expired & (status != 0))[:8].tolist()}"
        add("expired", expired.sum())
        print(f"{script.name} step {i} ({names[i]}, {out[i]['steps']} steps): status (0, 1) ({int((status == 0).sum())}, {int((status == 1).sum())}), expired {int(expired.sum())}, "
              f"rows per hit bit {[int(((hit & b) != 0).sum()) for b in HIT_BITS]}")
    if motions:
        both = [(int((out[i]["status"] == 0).sum()), int((out[i]["status"] == 1).sum())) for i in motions]
        assert any(a > 0 and b > 0 for a, b in both), f"{script.name}: no motion step left both status 0 and status 1: {both}"
        assert all(set(np.unique(out[i]["status"])) <= {0, 1} for i in motions)
    kills = [i for i in motions if names[i] == "motion_kill_compact"]
    if kills:
        kept = [(int((out[i]["slot"] >= 0).sum()), len(out[i]["slot"])) for i in kills]
        print(f"{script.name}: motion kills (kept, rows): {kept}")
        assert any(0 < k < n for k, n in kept), f"{script.name}: no motion kill both dropped and kept a row: {kept}"
        for i in kills:
            assert out[i]["counts"][0] == int((out[i]["slot"] >= 0).sum()) == int((out[i]["status"] >= 1).sum()) == twin[i][1]["live"]
            live = out[i]["counts"][0]  # the compacted rows: positions behind the live count are the fill, in front of it finite
            assert np.isnan(twin[i][1]["motion_xyz"][live:]).all() and np.isfinite(twin[i][1]["motion_xyz"][:live]).all()
    return seen


def check_liveness(script, twin):
    """the script did exercise the state it is about -- counted from the twin's recorded outputs, so that a script which never reaches the hidden state cannot pass empty"""
    names = [k for k, _ in script.steps]
    out = [t[0] for t in twin]
    if steps_of(script, ("shape", "diffuse", "motion")):
        FEATURE_SEEN[script.name] = feature_counts(script, twin)
        print(f"{script.name}: {FEATURE_SEEN[script.name]}")
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


def test_every_motion_mode_and_every_class_of_voxel_occurs_somewhere():
    """over the twin's passes of the scripts that shape, diffuse or step points (counted by check_liveness where the comparison above has run; a script it has not seen
    runs its twin's pass here): bit 1 and bit 16 under bounce, bit 2 under stick, bit 4 under kill, bit 8 somewhere, a row that expires by age; a diffuse with inactive
    voxels, and a diffuse_walls with solid voxels and unknowns"""
    total = {}
    for script in sq.SCRIPTS:
        if steps_of(script, ("shape", "diffuse", "motion")):
            seen = FEATURE_SEEN.get(script.name)
            if seen is None:
                seen = feature_counts(script, sq.twin_record(script.name))
            for k, v in seen.items():
                total[k] = total.get(k, 0) + v
    print(f"counts over the suite: {total}")
    for key in (("bounce", 1), ("bounce", 16), ("stick", 2), ("kill", 4), "expired", "diffuse steps with inactive voxels", "diffuse_walls steps with solid voxels and unknowns"):
        assert total.get(key, 0) > 0, (key, total)
    assert sum(v for k, v in total.items() if isinstance(k, tuple) and k[1] == 8) > 0, total
    assert not any(v for k, v in total.items() if isinstance(k, tuple) and k[0] == "free"), total  # (mode free looks at no collider)


def frame_shaped_against_the_mirrors():
    """one shape_controlled, one diffuse_walls and one motion_bounce of the twin's pass of frame_shaped, each on the state the twin captured in front of the step, every word"""
    import diffusion_cases as dc
    import point_motion_cases as mc
    import shaping_cases as shc
    from oracle_lib import OracleGrid, oracle_device
    from test_points_gpu import assert_same_bits, assert_words

    script = sq.BY_NAME["frame_shaped"]
    names = [k for k, _ in script.steps]
    twin = sq.twin_record(script.name)
    fields = sq.PROFILES[script.profile]

    def unlisted_kept(i, written):
        before, after = state_before(script, twin, i), twin[i][1]
        for k in after:
            if k not in written and not (k == "masks" and before[k] is None):
                assert np.array_equal(sq.as_words(after[k]), sq.as_words(before[k])), f"frame_shaped step {i} ({names[i]}) changed {k}"

    # the shape: the turbulence of the step's own rng, the weight from density before its decay
    i = names.index("shape_controlled")
    before, after = state_before(script, twin, i), twin[i][1]
    turbulence = sq._turbulence(np.random.default_rng(script.steps[i][1]), **sq.CONTROL)
    vel, out = shc.apply_mirror(dc.coords(before["origins"]), before["vel"], {"density": before["density"]}, sq.DT, turbulence, sq.DECAY)
    w = (before["density"] - np.float32(sq.CONTROL["control_lo"])) / np.float32(sq.CONTROL["control_hi"] - sq.CONTROL["control_lo"])
    print(f"frame_shaped step {i}: {turbulence['octaves']} octaves; weights (0, between, 1): {int((w <= 0).sum())}, {int(((w > 0) & (w < 1)).sum())}, {int((w >= 1).sum())}; "
          f"{int((words(vel) != words(before['vel'])).sum())} of {vel.size} velocity words move in the mirror")
    assert (w <= 0).any() and ((w > 0) & (w < 1)).any() and (w >= 1).any() and (words(vel) != words(before["vel"])).mean() > 0.25
    assert_words(after["vel"], vel, "frame_shaped's shape_controlled against shaping_cases.apply_mirror: vel")
    assert_words(after["density"], out["density"], "frame_shaped's shape_controlled against shaping_cases.apply_mirror: density")
    unlisted_kept(i, ("vel", "density"))
    # the diffuse: the captured masks and collision_sdf decide the unknowns, the walls and the faces
    i = names.index("diffuse_walls")
    before, after = state_before(script, twin, i), twin[i][1]
    active = active_of(before)
    want = dc.apply_mirror(before["origins"], {k: before[k] for k in ["vel"] + fields}, sq.DT, sq.VS, active=active, **sq.diffuse_arguments("diffuse_walls"))
    unknown, solid = dc.classes(len(active), active, before["collision_sdf"], True, 0.0)
    print(f"frame_shaped step {i}: {int(unknown.sum())} unknowns, {int(solid.sum())} solid voxels of {len(active)}; the mirror changes "
          f"{int((words(want['vel']) != words(before['vel'])).sum())} velocity words and {int((words(want['density']) != words(before['density'])).sum())} density words")
    assert unknown.any() and solid.any() and (words(want["density"]) != words(before["density"])).any() and (words(want["vel"]) != words(before["vel"])).any()
    for k in ["vel"] + fields:
        assert_words(after[k], want[k], f"frame_shaped's diffuse_walls against diffusion_cases.apply_mirror: {k}")
    unlisted_kept(i, ("vel", "density"))
    # the motion step (the device-semantics build of the oracle: the rows hold NaN and infinite positions and velocities; a NaN is equal to any NaN, as in
    # tests/test_point_motion_gpu.py's special values)
    i = names.index("motion_bounce")
    before, after = state_before(script, twin, i), twin[i]
    mode, _, spec = sq.MOTION_SPECS["motion_bounce"]
    steps = after[0]["steps"]
    assert names[i - 1] == "motion_load" and mode == "bounce" and not np.isfinite(before["motion_xyz"]).all() and not np.isfinite(before["motion_vel"]).all()
    G = OracleGrid(before["origins"], lib=oracle_device())
    inv_dx = float(np.float32(1.0) / np.float32(sq.VS))
    x, v, age, status, hit, _ = mc.motion_mirror(G, before["vel"], before["collision_sdf"], before["motion_xyz"], before["motion_vel"], before["motion_age"], sq.DT, inv_dx, steps,
                                                 mode, dict(spec, threshold=0.0))
    print(f"frame_shaped step {i}: {steps} steps; the mirror's status (0, 1) ({int((status == 0).sum())}, {int((status == 1).sum())}), rows per hit bit "
          f"{[int(((hit & b) != 0).sum()) for b in HIT_BITS]}, {int((words(x).reshape(-1, 3) != words(before['motion_xyz']).reshape(-1, 3)).any(1).sum())} rows moved")
    assert (hit & 1).any() and (hit & 16).any() and (hit == 0).any() and status.any() and not status.all()
    assert np.array_equal(after[0]["status"], status), f"status differs at rows {np.flatnonzero(after[0]['status'] != status)[:8].tolist()}"
    assert np.array_equal(after[0]["hit"], hit), f"hit differs at rows {np.flatnonzero(after[0]['hit'] != hit)[:8].tolist()}"
    for k, a in (("xyz", x), ("vel", v), ("age", age)):
        assert_same_bits(after[1]["motion_" + k], a, f"frame_shaped's motion_bounce against point_motion_cases.motion_mirror: {k}")
    unlisted_kept(i, ("motion_xyz", "motion_vel", "motion_age"))


def test_the_twin_equals_the_mirrors():
    """frame_points' trace_collide_push against points_collide_cases.collide_mirror, and its first neighbours_original against neighbour_cases.restate, each on the state
    the twin captured in front of the step: words for the positions, bytes for status and hit; bytes of count, density and push for the 1,500 points. Then frame_shaped's
    first shape_controlled against shaping_cases.apply_mirror, its first diffuse_walls against diffusion_cases.apply_mirror on the captured masks and collision_sdf, and its
    first motion_bounce against point_motion_cases.motion_mirror on the oracle's device-semantics build: every word of everything the step may write, and everything else
    of the captured state unchanged"""
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
    frame_shaped_against_the_mirrors()


def test_the_twin_is_deterministic():
    """two twin passes of a script give the same bytes: the comparison above is of the library, not of the harness"""
    script = sq.BY_NAME["frame_vcycle"]
    a, b = sq.twin_record(script.name), sq.run_twin(script)
    assert sq.first_difference(script, "twin", a, [(o, s, None) for o, s in b]) is None
