"""The harness of tests/test_streams_gpu.py, checked without a GPU: every entry point that takes a stream is a case or a stated exemption, and the guard bands and the
input comparison report what is planted in them."""
import os

import numpy as np
import pytest
import torch

import stream_cases as sc
from hnanosolver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_point_with_a_stream_is_a_case_or_exempt():
    """a new entry point with a `void* stream` parameter fails here until someone adds a case or states why it needs none"""
    declared = sc.stream_entry_points(open(os.path.join(ROOT, "include", "hns.h")).read())
    assert len(declared) == len(set(declared)) and len(declared) >= 50
    assert "hns_sim_substep" in declared and "hns_dev_pack_leaves" in declared and "hns_sim_regrid_seeded" in declared  # (the parser reads multi-line prototypes)
    assert "hns_grid_splat_points" not in declared and "hns_sim_timing" not in declared
    bound = [n for n in declared if n in _lib.SIGNATURES]
    assert bound == declared, sorted(set(declared) - set(bound))  # every one has a prototype in _lib.py
    for name in declared:  # (the stream is passed as an address)
        assert _lib._vp in _lib.SIGNATURES[name][1], name
    undecided = [n for n in declared if n not in sc.CASES and n not in sc.EXEMPT]
    assert not undecided, f"entry points with a stream parameter that are neither in stream_cases.CASES nor in EXEMPT: {undecided}"
    assert not set(sc.CASES) & set(sc.EXEMPT)
    assert not (set(sc.CASES) | set(sc.EXEMPT)) - set(declared), "a case or exemption for something include/hns.h does not declare with a stream"


def test_exemptions_are_the_dist_calls_and_the_timing_helper():
    assert all(n.startswith("hns_dist_") or n == "hns_dev_time_rbgs" for n in sc.EXEMPT)
    assert all(isinstance(r, str) and len(r) > 20 and "\n" not in r for r in sc.EXEMPT.values())


def test_the_table_states_a_source_for_every_case():
    for name, e in sc.CASES.items():
        assert e.level in ("kernel", "sim", "operator") and e.variants and e.grids and set(e.grids) <= set(sc.GRIDS), name
        assert "null stream" in e.source, name
    ids = sc.variants("kernel") + sc.variants("sim") + sc.variants("operator")
    assert len(ids) == len(set(ids)) and {n for n, _, _ in ids} == set(sc.CASES)


SPECS = {"vec": ((5 * 512, 3), np.float32), "status": ((1031,), np.uint8), "flt": ((3 * 512,), np.float32), "count": ((1,), np.int64)}


def test_slab_layout():
    s = sc.Slab(torch, SPECS)
    assert sc.GUARD_BYTES == 2 * 512 * 3 * 4 and sc.GUARD_BYTES % 256 == 0
    assert s.words.numel() * 4 == s.bytes.numel()
    end = 0
    for (name, start, n), (shape, dtype) in zip(s.extents, SPECS.values()):
        v = s.views[name]
        assert tuple(v.shape) == tuple(shape) and v.is_contiguous() and v.numel() * v.element_size() == n
        assert start % 256 == 0 and start - end >= sc.GUARD_BYTES  # aligned, a whole guard in front
        assert v.data_ptr() - s.bytes.data_ptr() == start  # a view of the slab, not a copy
        end = start + n
    assert s.bytes.numel() - end >= sc.GUARD_BYTES
    s.check("fresh")
    for v in s.views.values():  # writing every byte of every view leaves the guards alone
        sc.sentinel(v)
    s.check("views written")
    assert int(s.views.vec.view(torch.int32)[0, 0]) == sc._signed(sc.OUT_WORD) and int(s.views.status[-1]) == sc.OUT_BYTE


@pytest.mark.parametrize("where", ["leading", "trailing", "past_bytes", "first", "last"])
def test_slab_reports_a_planted_overwrite(where):
    s = sc.Slab(torch, SPECS)
    _, start, n = s.extents[2]  # flt
    flat = s.bytes
    if where == "leading":  # one word in front of flt
        flat[start - 4:start] = 0
        hint = "leading guard of flt, 4 bytes before"
    elif where == "trailing":
        flat[start + n:start + n + 4] = 0
        hint = "trailing guard of flt, 0 bytes past"
    elif where == "past_bytes":  # the byte behind a 1031-byte view: inside the padding to the next 256 bytes
        _, s1, n1 = s.extents[1]
        flat[s1 + n1] = 0
        hint = "trailing guard of status, 0 bytes past"
    elif where == "first":
        flat[0:4] = 0
        hint = "leading guard of vec"
    else:
        flat[-4:] = 0
        hint = "trailing guard of count"
    with pytest.raises(AssertionError) as e:
        s.check("planted")
    assert hint in str(e.value) and str(e.value).count("guard of") == (2 if where in ("leading", "trailing", "past_bytes") else 1), str(e.value)


def test_inputs_unchanged_reports_a_planted_word():
    rng = np.random.default_rng(0)
    staging = {"vel": rng.standard_normal((1024, 3)).astype(np.float32), "p": rng.standard_normal(1024).astype(np.float32), "ids": np.arange(7, dtype=np.int32)}
    after = {k: torch.from_numpy(v.copy()) for k, v in staging.items()}
    sc.assert_inputs_unchanged(after, staging, what="clean")
    after["p"].view(torch.int32)[513] ^= 1  # one bit of one word
    with pytest.raises(AssertionError, match="input p was written"):
        sc.assert_inputs_unchanged(after, staging, what="planted")
    sc.assert_inputs_unchanged(after, staging, inplace=("p",), what="p is documented as in place")
    after["vel"][3, 1] = float("nan")  # NaN against a number, and NaN against NaN compares as words
    with pytest.raises(AssertionError, match="input vel was written"):
        sc.assert_inputs_unchanged(after, staging, inplace=("p",), what="planted")
    nan = {"x": np.full(4, sc.NAN_WORD, dtype=np.uint32).view(np.float32)}
    sc.assert_inputs_unchanged({"x": torch.from_numpy(nan["x"].copy())}, nan, what="NaN words")


def test_poison_words():
    t = torch.zeros(6, 3)
    sc.fill_words(t, sc.NAN_WORD)
    assert bool(torch.isnan(t).all()) and int(t.view(torch.int32)[0, 0]) == sc.NAN_WORD
    b = torch.zeros(5, dtype=torch.uint8)
    sc.fill_words(b, sc.OUT_BYTE)
    assert b.tolist() == [0xAB] * 5
