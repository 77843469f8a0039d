"""hns_point_motion_* without a GPU: exported, declared and bound; create without a device gives HNS_ERR_NO_DEVICE; every refusal of a number or of the spec returns
HNS_ERR_INVALID_ARGUMENT with the call and the argument in the message before any object is looked at (null objects serve); the header compiles as strict C99 and a C
program fills the spec; and the three coverage tables' parsers (tests/stream_cases.py, tests/layout_cases.py, the prefixes of tests/test_sequence_cases.py) see none of
the calls: the object owns its arrays and hands pointers out, no call takes a caller's data pointer or a `void* stream`. What step computes is held word for word to the
mirror on the MI355X (tests/test_point_motion_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hnanosolver_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_point_motion_create", "hns_point_motion_destroy", "hns_point_motion_set_stream", "hns_point_motion_get", "hns_point_motion_step")
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


def header():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    decl = re.search(r"^(?:int|void|hns_point_motion\*)\s+%s\s*\(([^;]*)\);" % name, header(), re.M | re.S)
    assert decl, f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1  # one ctypes argument per parameter of the declaration


def test_the_structs_and_the_modes_are_the_headers():
    h = header()
    for k, v in (("FREE", 0), ("STICK", 1), ("BOUNCE", 2), ("KILL", 3)):
        assert re.search(r"^#define HNS_MOTION_%s %d\b" % (k, v), h, re.M) and getattr(_lib, "HNS_MOTION_" + k) == v
    assert device.MOTION_MODES == {"free": 0, "stick": 1, "bounce": 2, "kill": 3}
    body = re.search(r"typedef struct hns_point_motion_spec \{(.*?)\} hns_point_motion_spec;", h, re.S).group(1)
    members = re.findall(r"^\s*(int|float)\s+(\w+)(?:\[3\])?;", body, re.M)
    assert [n for _, n in members] == [n for n, _ in _lib.hns_point_motion_spec._fields_]
    assert [n for n, _ in _lib.hns_point_motion_spec._fields_] == ["mode", "gravity", "drag", "restitution", "friction", "max_age", "threshold", "skin", "iterations"]
    assert C.sizeof(_lib.hns_point_motion_spec) == 44
    body = re.search(r"typedef struct hns_point_motion_info \{(.*?)\} hns_point_motion_info;", h, re.S).group(1)
    members = re.findall(r"^\s*(?:uint64_t|float\*|unsigned char\*)\s+(\w+);", body, re.M)
    assert members == [n for n, _ in _lib.hns_point_motion_info._fields_] == ["capacity", "xyz", "vel", "age", "status", "hit"]
    assert C.sizeof(_lib.hns_point_motion_info) == 48


def test_header_states_the_arithmetic_line_by_line():
    h = header()
    comment = h[h.index("POINTS WITH A VELOCITY OF THEIR OWN"): h.index("typedef struct hns_point_motion hns_point_motion;")]
    for word in ("inv_dx = 1.0f / voxel_size", "s = dt * inv_dx", "k = drag * dt", "r = 1.0f / (1.0f + k)", "gd.c = dt * gravity.c", "ft = 1.0f - friction",
                 "t.c = k * u.c; t.c = v.c + t.c; v.c = t.c * r", "v.c = v.c + gd.c", "m.c = s * v.c; x1.c = x0.c + m.c", "age = age + dt", "STICK", "KILL", "BOUNCE",
                 "vn = (v.x*n.x + v.y*n.y) + v.z*n.z", "w.c = vn * n.c; vt.c = v.c - w.c; a = restitution * vn", "p.c = ft * vt.c; q.c = a * n.c; v.c = p.c - q.c",
                 "hit |= 16", "a = a + skin", "-x, +x, -y, +y, -z, +z", "age < max_age", "mirrored in", "hns_dist_*", "no leaves"):
        assert word in comment, word


def spec(**over):
    good = dict(mode=2, gravity=(0.0, -9.8, 0.0), drag=2.0, restitution=0.5, friction=0.25, max_age=1.0, threshold=0.0, skin=0.0625, iterations=3)
    s = {**good, **over}
    return _lib.hns_point_motion_spec(s["mode"], (C.c_float * 3)(*s["gravity"]), s["drag"], s["restitution"], s["friction"], s["max_age"], s["threshold"], s["skin"],
                                      s["iterations"])


def test_every_refusal_of_a_number_comes_before_the_objects_are_looked_at():
    lib = _lib.load_library()
    nan, inf = float("nan"), float("inf")

    def call(n=5, dt=0.04, vs=1.0 / 24, steps=1, null_spec=False, **over):
        sp = spec(**over)
        return lambda: lib.hns_point_motion_step(None, None, n, dt, vs, steps, None if null_spec else C.byref(sp))

    rows = [
        (call(null_spec=True), "spec"), (call(n=2 ** 31), "2^31"), (call(steps=0), "steps"), (call(steps=-1), "steps"), (call(dt=nan), "dt"),
        (call(vs=0.0), "voxel_size"), (call(vs=-1.0), "voxel_size"), (call(vs=inf), "voxel_size"), (call(vs=nan), "voxel_size"),
        (call(mode=-1), "mode"), (call(mode=4), "mode"),
        (call(gravity=(nan, 0, 0)), "gravity"), (call(gravity=(0, inf, 0)), "gravity"), (call(gravity=(0, 0, -inf)), "gravity"),
        (call(drag=nan), "drag"), (call(drag=inf), "drag"), (call(drag=-0.5), "drag"),
        (call(restitution=nan), "restitution"), (call(restitution=-0.01), "restitution"), (call(restitution=1.01), "restitution"),
        (call(friction=nan), "friction"), (call(friction=-0.01), "friction"), (call(friction=1.01), "friction"),
        (call(max_age=nan), "max_age"), (call(max_age=0.0), "max_age"), (call(max_age=-1.0), "max_age"),
        (call(threshold=nan), "threshold"), (call(threshold=inf), "threshold"), (call(threshold=-inf), "threshold"),
        (call(skin=nan), "skin"), (call(skin=inf), "skin"), (call(skin=-0.001), "skin"),
        (call(iterations=0), "iterations"), (call(iterations=9), "iterations"), (call(mode=0, iterations=0), "iterations"), (call(mode=1, iterations=9), "iterations"),
        (call(mode=3, iterations=-1), "iterations"),
        # n == 0 does not excuse a number
        (call(n=0, steps=0), "steps"), (call(n=0, mode=4), "mode"), (call(n=0, null_spec=True), "spec"),
        # every number in range (+inf max_age, the ends of [0, 1], a negative dt, a zero drag and skin): the null object is what is refused
        (call(max_age=inf, restitution=0.0, friction=1.0, dt=-0.04, drag=0.0, skin=0.0, iterations=8, mode=0), "null point motion"),
        (call(restitution=1.0, friction=0.0, iterations=1), "null point motion"),
    ]
    wrong = []
    for i, (fn, word) in enumerate(rows):
        lib.hns_set_option(b"rbgs", None)  # (a call that succeeds: whatever it leaves in hns_last_error(), the text read below is this row's)
        code, text = fn(), lib.hns_last_error().decode()
        if code != BAD or not text.startswith("hns_point_motion_step:") or word not in text:
            wrong.append(f"row {i} (expects {word!r}): got {code} {text!r}")
    assert not wrong, "\n".join(wrong)


def test_null_objects_and_a_capacity_beyond_the_bound_are_refused_under_the_calls_names():
    lib = _lib.load_library()
    info = _lib.hns_point_motion_info()
    for fn, who, word in ((lambda: lib.hns_point_motion_get(None, C.byref(info)), "hns_point_motion_get:", "null point motion"),
                          (lambda: lib.hns_point_motion_set_stream(None, None), "hns_point_motion_set_stream:", "null point motion")):
        lib.hns_set_option(b"rbgs", None)
        assert fn() == BAD
        text = lib.hns_last_error().decode()
        assert text.startswith(who) and word in text, text
    err = C.c_int(7)
    assert not lib.hns_point_motion_create(2 ** 31, C.byref(err)) and err.value == BAD
    text = lib.hns_last_error().decode()
    assert text.startswith("hns_point_motion_create:") and "capacity" in text and "2^31" in text
    assert not lib.hns_point_motion_create(2 ** 31, None)  # (a null err is allowed)
    lib.hns_point_motion_destroy(None)  # (a null object is allowed)


def test_create_without_a_device_is_no_device():
    lib = _lib.load_library()
    if lib.hns_device_count() == 0:  # (with a device, tests/test_point_motion_gpu.py creates objects on it)
        err = C.c_int(0)
        assert not lib.hns_point_motion_create(16, C.byref(err)) and err.value == _lib.HNS_ERR_NO_DEVICE
        text = lib.hns_last_error().decode()
        assert text.startswith("hns_point_motion_create:") and "no HIP device" in text
        with pytest.raises(Exception, match="no HIP device"):
            device.PointMotion(16)


def test_python_class_refuses_before_the_library_is_reached():
    with pytest.raises(ValueError, match="negative"):
        device.PointMotion(-1)
    assert callable(device.Sim.point_motion) and callable(device.PointMotion.step) and callable(device.PointMotion.close)
    assert hasattr(device.PointMotion, "__enter__") and hasattr(device.PointMotion, "__exit__")
    for name in ("xyz", "vel", "age", "status", "hit"):
        assert isinstance(getattr(device.PointMotion, name), property)


def test_header_is_plain_c99_and_a_c_program_fills_the_spec(tmp_path):
    src = tmp_path / "motion_abi.c"
    src.write_text('#include "hns.h"\n#include <stdio.h>\n#include <string.h>\nint main(void) {\n'
                   '  int err = 0;\n  hns_point_motion_info info;\n'
                   '  hns_point_motion_spec sp = {HNS_MOTION_BOUNCE, {0.0f, -9.8f, 0.0f}, 2.0f, 0.5f, 0.25f, 1.0f, 0.0f, 0.0625f, 3};\n'
                   '  if (sizeof sp != 44 || HNS_MOTION_FREE != 0 || HNS_MOTION_STICK != 1 || HNS_MOTION_KILL != 3) return 1;\n'
                   '  if (hns_point_motion_get(NULL, &info) != HNS_ERR_INVALID_ARGUMENT) return 2;\n'
                   '  sp.iterations = 9;\n'
                   '  if (hns_point_motion_step(NULL, NULL, 4, 0.04f, 0.125f, 1, &sp) != HNS_ERR_INVALID_ARGUMENT || !strstr(hns_last_error(), "iterations")) return 3;\n'
                   '  if (hns_point_motion_create((uint64_t)1 << 31, &err) || err != HNS_ERR_INVALID_ARGUMENT) return 4;\n'
                   '  hns_point_motion_destroy(NULL);\n  printf("motion abi ok\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "motion_abi")
    libdir = os.path.dirname(_lib.library_path())
    b = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lhns",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "motion abi ok" in r.stdout, f"{r.returncode} {r.stdout} {r.stderr}"


def test_the_coverage_tables_parsers_see_none_of_the_calls():
    """the header as it now stands goes through the parsers of the stream and layout coverage tests: no call has a `void* stream` parameter or a data-pointer
    parameter, so those two tables do not see them. The sequence vocabulary does: every call starts with one of its prefixes and is an operation's or the runners'
    symbol there, or a stated exemption"""
    import layout_cases
    import stream_cases
    import sequence_cases
    from test_sequence_cases import PREFIXES

    h = header()
    streamed, pointed = stream_cases.stream_entry_points(h), layout_cases.data_pointer_entry_points(h)
    assert "hns_dev_trace_points_collide" in streamed and "hns_dev_trace_points_collide" in pointed  # (the parsers do see the header)
    for name in SYMBOLS:
        assert name not in streamed and name not in pointed and name.startswith(PREFIXES), name
        used = name in sequence_cases.RUNNER_SYMBOLS or any(name in o.symbols for o in sequence_cases.OPS.values())
        assert used != (name in sequence_cases.EXEMPT), name
        assert name not in stream_cases.CASES and name not in layout_cases.LAYOUT_CASES
