"""The harness of tests/test_operand_layout_gpu.py, checked without a GPU: every entry point that takes a device data pointer is a case or a stated exemption, the slab
puts every view where a layout says, and the guard bands report what a kernel with a rounded-down or too wide access would leave behind."""
import os

import numpy as np
import pytest
import torch

import layout_cases as lc
import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hns.h")).read()


def test_every_entry_point_with_a_data_pointer_is_a_case_or_exempt():
    """a new entry point with a `float*` (or any other data pointer) parameter fails here until someone adds a layout case or states why it needs none"""
    declared = lc.data_pointer_entry_points(HEADER)
    assert len(declared) == len(set(declared)) and len(declared) >= 80
    for name in ("hns_dev_advect_scalars", "hns_point_order_gather", "hns_dev_field_stats", "hns_sim_regrid_seeded", "hns_point_population_compact", "hns_dev_splat_points"):
        assert name in declared, name  # (float* const*, void* rows, hns_stats*, multi-line prototypes)
    for name in ("hns_sim_substep", "hns_grid_destroy", "hns_set_option", "hns_sim_upload", "hns_point_order_set_stream", "hns_point_order_cells", "hns_sim_deactivate"):
        assert name not in declared, name  # (handles, text, struct specs, a stream, a pointer the library hands OUT)
    undecided = [n for n in declared if n not in lc.LAYOUT_CASES and n not in lc.LAYOUT_EXEMPT]
    assert not undecided, f"entry points with a data-pointer parameter that are neither in layout_cases.LAYOUT_CASES nor in LAYOUT_EXEMPT: {undecided}"
    assert not set(lc.LAYOUT_CASES) & set(lc.LAYOUT_EXEMPT)
    assert not (set(lc.LAYOUT_CASES) | set(lc.LAYOUT_EXEMPT)) - set(declared), "a case or exemption for something include/hns.h does not declare with a data pointer"


def test_a_new_prototype_with_a_float_pointer_is_noticed():
    more = HEADER.replace("#ifdef __cplusplus\n}", "int hns_dev_new_thing(hns_grid*, const float* field,\n  float* out, void* stream);\n#ifdef __cplusplus\n}", 1)
    assert "hns_dev_new_thing" in lc.data_pointer_entry_points(more) and "hns_dev_new_thing" not in lc.LAYOUT_CASES and "hns_dev_new_thing" not in lc.LAYOUT_EXEMPT


def test_every_sentence_about_aliasing_has_its_case():
    """a new "may alias" in include/hns.h needs an in-place case, a new "must not alias" / "not aliasing" a refusal case (tests/test_operand_layout_gpu.py)"""
    assert lc.alias_sentences(HEADER, r"may alias") == set(lc.MAY_ALIAS)
    assert lc.alias_sentences(HEADER, r"must not alias|not aliasing") == set(lc.MUST_NOT_ALIAS)
    more = HEADER.replace("#ifdef __cplusplus\n}", "/* out must not alias in */\nint hns_dev_new_thing(const float* in, float* out);\n#ifdef __cplusplus\n}", 1)
    assert "hns_dev_new_thing" in lc.alias_sentences(more, r"must not alias|not aliasing")


def test_exemptions_state_one_of_the_four_reasons():
    assert set(lc.LAYOUT_EXEMPT.values()) <= set(lc.REASONS)
    for name, reason in lc.LAYOUT_EXEMPT.items():
        assert (reason == lc.DIST) == name.startswith("hns_dist_"), name
        assert (reason == lc.TIMING) == (name == "hns_dev_time_rbgs"), name
    assert all(len(r) > 20 and "\n" not in r for r in lc.REASONS)


def test_the_table_holds_every_kernel_level_stream_case_as_it_is():
    kernel = {n: e for n, e in sc.CASES.items() if e.level == "kernel"}
    assert len(kernel) == 22
    for name, e in kernel.items():
        assert lc.LAYOUT_CASES[name] is e, name  # the same builders, grids and expectations
    for name, e in lc.LAYOUT_CASES.items():
        assert e.variants and e.grids and set(e.grids) <= {"scattered", "plume"}, name
    ids = lc.variants()
    assert len(ids) == len(set(ids)) and {n for n, _, _ in ids} == set(lc.LAYOUT_CASES)
    for name in ("hns_point_order_gather", "hns_point_order_scatter"):
        assert set(lc.LAYOUT_CASES[name].variants) == {f"rows_of_{b}" for b in (4, 12, 16, 64)}
    assert set(lc.LAYOUT_CASES["hns_point_population_compact"].variants) == {f"rows_of_{b}{f}" for b in (4, 12, 16, 64) for f in ("", "_fill")}


OPERANDS = [("vel", np.float32), ("p", np.float32), ("masks", np.uint8), ("out", np.float32), ("rejected", np.int64), ("status", np.uint8), ("rec", np.uint8), ("hit", np.uint8),
            ("ids", np.int32), ("flags", np.uint8), ("more", np.float32)]


def test_skews_of_both_layouts():
    assert lc.skews("plus4", OPERANDS) == {"vel": 4, "p": 4, "masks": 1, "out": 4, "rejected": 8, "status": 1, "rec": 8, "hit": 1, "ids": 4, "flags": 1, "more": 4}
    assert lc.skews("mixed", OPERANDS) == {"vel": 12, "p": 8, "masks": 3, "out": 4, "rejected": 8, "status": 2, "rec": 8, "hit": 1, "ids": 12, "flags": 3, "more": 8}


SPECS = {"vec": ((5 * 512, 3), np.float32), "status": ((1031,), np.uint8), "flt": ((3 * 512,), np.float32), "count": ((1,), np.int64), "hit": ((1031,), np.uint8),
         "ids": ((7,), np.int32)}
WANT = {"plus4": {"vec": 4, "status": 1, "flt": 4, "count": 8, "hit": 1, "ids": 4}, "mixed": {"vec": 12, "status": 3, "flt": 8, "count": 8, "hit": 2, "ids": 4}}


def _slab(layout):
    return sc.Slab(torch, SPECS, skew=lc.skews(layout, [(k, d) for k, (_, d) in SPECS.items()]))


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_slab_layout_under_a_skew(layout):
    s = _slab(layout)
    end = 0
    for (name, start, n), (shape, dtype) in zip(s.extents, SPECS.values()):
        v = s.views[name]
        assert tuple(v.shape) == tuple(shape) and v.is_contiguous() and v.numel() * v.element_size() == n
        assert start % 256 == WANT[layout][name], (name, start % 256)
        assert start - end >= sc.GUARD_BYTES + WANT[layout][name]  # a whole guard in front of the slot, and the skipped bytes
        assert v.data_ptr() - s.bytes.data_ptr() == start
        end = start + n
    assert s.bytes.numel() - end >= sc.GUARD_BYTES
    s.check("fresh")
    for v in s.views.values():  # writing every byte of every view leaves the guards alone, the skipped bytes among them
        sc.sentinel(v)
    s.check("views written")
    host = s.bytes.numpy()
    for name, start, n in s.extents:
        gap = host[start - WANT[layout][name]:start]
        assert np.array_equal(gap, np.full(256, sc.GUARD_WORD, "<u4").view(np.uint8)[:len(gap)]), name  # (the slot starts at a multiple of 256: the pattern's phase is 0)


@pytest.mark.parametrize("layout", lc.LAYOUTS)
@pytest.mark.parametrize("view", ["vec", "flt", "status", "ids"])
def test_slab_reports_a_byte_in_the_skew_gap(layout, view):
    s = _slab(layout)
    start = {n: st for n, st, _ in s.extents}[view]
    s.bytes[start - 1] ^= 0xFF  # the last skipped byte
    with pytest.raises(AssertionError, match=f"leading guard of {view}, 1 bytes before its start"):
        s.check("planted")


@pytest.mark.parametrize("layout", lc.LAYOUTS)
@pytest.mark.parametrize("view", ["vec", "flt", "status", "ids"])
def test_slab_reports_a_16_byte_write_at_the_start_rounded_down(layout, view):
    """what a kernel leaves that takes `pointer & ~15` for the first 16-byte piece of an operand"""
    s = _slab(layout)
    start = {n: st for n, st, _ in s.extents}[view]
    down = start & ~15
    assert down < start
    s.bytes[down:down + 16] = 0
    with pytest.raises(AssertionError, match=f"leading guard of {view}, {start - down} bytes before its start"):
        s.check("planted")
