"""Mixed call sequences on one device-resident sim against a twin with no hidden state (tests/sequence_cases.py states the vocabulary, the two runners and the scripts;
tests/test_sequence_cases.py holds the scripts' coverage conditions without a GPU).

The twin's pass of a script runs first, every step on a sim, an order and a population of its own that are opened from the documented state alone, with lookahead = 0 and
the pool of device memory filled with a non-zero byte. Then ONE sim runs the script from its first step to its last, once with lookahead = auto and once with
lookahead = 1, and after every step everything the step returned and the full downloaded state must be the twin's, byte for byte. Nothing here is a tolerance."""
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


def test_the_twin_is_deterministic():
    """two twin passes of a script give the same bytes: the comparison above is of the library, not of the harness"""
    script = sq.BY_NAME["frame_vcycle"]
    a, b = sq.twin_record(script.name), sq.run_twin(script)
    assert sq.first_difference(script, "twin", a, [(o, s, None) for o, s in b]) is None
