"""hns_dev_trace_points_collide and hns_sim_trace_points_collide without a GPU: exported, declared and bound; every refusal of an argument returns
HNS_ERR_INVALID_ARGUMENT with the call and the argument in the message before the grid's device tables are looked at (a host-only grid serves); n == 0 is accepted with
null pointers; the Python mirrors refuse an unknown mode. What the calls compute is held word for word to the mirror on the MI355X (tests/test_points_collide_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hnanosolver_amd import _lib, api, device, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_dev_trace_points_collide", "hns_sim_trace_points_collide")
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


def header():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    assert re.search(r"^int\s+%s\s*\(" % name, header(), re.M), f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header(), re.M | re.S).group(1)
    assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1  # one ctypes argument per parameter of the declaration
    assert C.POINTER(_lib.hns_point_collision) in _lib.SIGNATURES[name][1]


def test_the_spec_and_the_modes_are_the_headers():
    h = header()
    for k, v in (("STOP", 1), ("PUSH", 2), ("KILL", 3)):
        assert re.search(r"^#define HNS_COLLIDE_%s %d$" % (k, v), h, re.M) and getattr(_lib, "HNS_COLLIDE_" + k) == v
    body = re.search(r"typedef struct hns_point_collision \{(.*?)\} hns_point_collision;", h, re.S).group(1)
    members = re.findall(r"^\s*(int|float)\s+(\w+);", body, re.M)
    assert members == [("int", "mode"), ("float", "threshold"), ("float", "skin"), ("int", "iterations")]
    assert [(n, t) for n, t in _lib.hns_point_collision._fields_] == [("mode", C.c_int), ("threshold", C.c_float), ("skin", C.c_float), ("iterations", C.c_int)]
    assert C.sizeof(_lib.hns_point_collision) == 16
    assert device.COLLIDE_MODES == {"stop": 1, "push": 2, "kill": 3}


def test_header_states_the_arithmetic_and_that_the_calls_are_not_mirrored_in_the_partitioned_sim():
    h = header()
    comment = h[h.index("Points through the velocity against a collision SDF"): h.index("int hns_dev_trace_points_collide")]
    for word in ("STOP", "KILL", "PUSH", "a = a + skin", "-x, +x, -y, +y, -z, +z", "2.4e-38f", "mirrored in hns_dist_*"):
        assert word in comment, word
    assert "mirrored in hns_dist_*" in h[: h.index("int hns_sim_trace_points_collide")].rsplit("/*", 1)[1]


def test_every_argument_refusal_comes_before_the_device_is_looked_at():
    lib = _lib.load_library()
    o = fields.dense_leaves(16)
    h = api.create_grid_from_leaves(o, 1.0 / 16, _lib.HNS_GRID_HOST_ONLY)
    n, npts = len(o) * 512, 5
    vel, sdf = np.ones((n, 3), np.float32), np.full(n, -1.0, np.float32)
    xyz = np.full((npts, 3), 3.25, np.float32)
    status, hit = np.full(npts, 9, np.uint8), np.full(npts, 9, np.uint8)
    V, S, X, ST, H = vel.ctypes.data, sdf.ctypes.data, xyz.ctypes.data, status.ctypes.data, hit.ctypes.data
    nan, inf = float("nan"), float("inf")
    good = dict(mode=2, threshold=0.0, skin=0.0625, iterations=2)

    def call(grid=h.ptr, vel=V, sdf=S, p=X, count=npts, dt=0.04, inv=16.0, order=2, steps=1, status_=ST, hit_=H, null_spec=False, **spec):
        c = _lib.hns_point_collision(*[{**good, **spec}[k] for k in ("mode", "threshold", "skin", "iterations")])
        return lambda: lib.hns_dev_trace_points_collide(grid, vel, sdf, p, count, dt, inv, order, steps, None if null_spec else C.byref(c), status_, hit_, None)

    rows = [
        # everything hns_dev_trace_points refuses
        (call(grid=None), "null grid"), (call(p=None), "xyz"), (call(vel=None), "vel3"), (call(order=3), "order"), (call(order=0), "order"), (call(steps=0), "steps"),
        (call(steps=-2), "steps"), (call(dt=nan), "dt"), (call(inv=0.0), "inv_dx"), (call(inv=-16.0), "inv_dx"), (call(inv=inf), "inv_dx"), (call(inv=nan), "inv_dx"),
        (call(count=2 ** 31), "2^31"), (call(status_=X), "status is xyz"), (call(vel=X), "vel3 is xyz"), (call(status_=V), "status is vel3"),
        # the spec
        (call(null_spec=True), "spec"), (call(mode=0), "mode"), (call(mode=4), "mode"), (call(mode=-1), "mode"), (call(threshold=nan), "threshold"),
        (call(threshold=inf), "threshold"), (call(threshold=-inf), "threshold"), (call(skin=nan), "skin"), (call(skin=inf), "skin"), (call(skin=-0.001), "skin"),
        (call(iterations=0), "iterations"), (call(iterations=9), "iterations"), (call(mode=1, iterations=0), "iterations"), (call(mode=3, iterations=9), "iterations"),
        # the SDF and the aliases
        (call(sdf=None), "sdf"), (call(sdf=X), "sdf is xyz"), (call(sdf=V), "sdf is vel3"), (call(status_=S), "status is sdf"), (call(hit_=X), "hit is xyz"),
        (call(hit_=V), "hit is vel3"), (call(hit_=S), "hit is sdf"), (call(hit_=ST), "hit is status"),
    ]
    wrong = []
    for i, (fn, word) in enumerate(rows):
        lib.hns_set_option(b"rbgs", None)  # (a call that succeeds: whatever it leaves in hns_last_error(), the text read below is this row's)
        code, text = fn(), lib.hns_last_error().decode()
        if code != BAD or not text.startswith("hns_dev_trace_points_collide:") or word not in text:
            wrong.append(f"row {i} (expects {word!r}): got {code} {text!r}")
    assert not wrong, "\n".join(wrong)
    # the sim form: no sim exists without a device, and a null sim is refused under the call's own name
    c = _lib.hns_point_collision(2, 0.0, 0.0625, 2)
    code = lib.hns_sim_trace_points_collide(None, X, npts, 0.04, 1.0 / 16, 2, 1, C.byref(c), ST, H, None)
    assert code in (BAD, _lib.HNS_ERR_NO_DEVICE) and lib.hns_last_error().decode().startswith("hns_sim_trace_points_collide:")
    # n == 0: nothing is launched and no pointer is looked at, whatever the mode
    for mode in (1, 2, 3):
        assert call(vel=None, sdf=None, p=None, count=0, status_=None, hit_=None, mode=mode)() == 0
    # ... but the numbers and the spec, which is a host struct, are checked whatever n (include/hns.h), as hns_dev_trace_points checks order and steps
    for fn, word in ((call(count=0, null_spec=True), "spec"), (call(count=0, mode=4), "mode"), (call(count=0, iterations=9), "iterations"), (call(count=0, order=3), "order")):
        assert fn() == BAD and word in lib.hns_last_error().decode(), word
    # a well-formed call reaches the device check: there is no CPU fallback
    if lib.hns_device_count() == 0:
        assert call()() == _lib.HNS_ERR_NO_DEVICE and "no CPU fallback" in lib.hns_last_error().decode()
    assert (xyz == np.float32(3.25)).all() and (status == 9).all() and (hit == 9).all()


def test_python_mirrors_exist_and_refuse_an_unknown_mode():
    assert callable(device.trace_points_collide)
    with pytest.raises(ValueError, match="bogus"):
        device.Sim.trace(object(), None, dt=0.04, voxel_size=1.0 / 16, collide="bogus")
    with pytest.raises(ValueError, match="bogus"):
        device.trace_points_collide(None, None, None, None, 0.04, 16.0, mode="bogus")
    with pytest.raises(TypeError):
        device.trace_points_collide(None, None, None, None, 0.04, 16.0)  # the mode has no default


def test_both_calls_are_stream_cases_and_the_sim_form_is_decided_for_the_sequences():
    """the feature's entries stand in the tables themselves: both calls are cases of the late-stream harness (tests/stream_cases.py), and the sim's form is an operation
    of the call-sequence vocabulary (tests/sequence_cases.py) in every mode, held by a committed script, and no exemption"""
    import sequence_cases
    import stream_cases

    declared = stream_cases.stream_entry_points(header())
    for name in SYMBOLS:
        assert name in declared and "null stream" in stream_cases.CASES[name].source and "collide_mirror" in stream_cases.CASES[name].source
        assert (name, stream_cases.COLLIDE_VARIANT, "scattered") in stream_cases.variants(stream_cases.CASES[name].level)
        assert name not in stream_cases.EXEMPT
    name = "hns_sim_trace_points_collide"
    assert name not in sequence_cases.EXEMPT
    ops = {k for k, o in sequence_cases.OPS.items() if name in o.symbols}
    assert ops == {"trace_collide_stop", "trace_collide_push", "trace_collide_kill_compact"}
    assert {sequence_cases.COLLIDE_SPECS[k][0] for k in ops} == set(device.COLLIDE_MODES)
    for k in ops:
        assert [s.name for s in sequence_cases.SCRIPTS if k in [n for n, _ in s.steps]], f"no committed script holds {k}"


@pytest.mark.gpu
def test_a_sim_without_collision_sdf_is_refused():
    import torch

    lib = _lib.load_library()
    o = fields.dense_leaves(16)
    g = api.create_grid_from_leaves(o, 1.0 / 16)
    s = device.Sim(g, ["density"])
    xyz = torch.full((5, 3), 3.25, device="cuda")
    c = _lib.hns_point_collision(1, 0.0, 0.0625, 2)
    assert lib.hns_sim_trace_points_collide(s._ptr, xyz.data_ptr(), 5, 0.04, 1.0 / 16, 2, 1, C.byref(c), None, None, None) == BAD
    text = lib.hns_last_error().decode()
    assert text.startswith("hns_sim_trace_points_collide:") and "collision_sdf" in text
    with pytest.raises(ValueError, match="collision_sdf"):  # (HNS_ERR_INVALID_ARGUMENT surfaces as ValueError)
        s.trace(xyz, dt=0.04, voxel_size=1.0 / 16, collide="stop")
    with pytest.raises(ValueError, match="bogus"):
        s.trace(xyz, dt=0.04, voxel_size=1.0 / 16, collide="bogus")
    torch.cuda.synchronize()
    assert (xyz.cpu().numpy() == np.float32(3.25)).all()
    s.close()
