"""hns_shaping_* without a GPU: exported, declared and bound; the three structs are the header's; the header states the arithmetic line by line; create without a
device gives HNS_ERR_NO_DEVICE; every refusal of a number or of a spec returns HNS_ERR_INVALID_ARGUMENT with the call and the argument in the message before any object is
looked at (null objects serve); the header compiles as strict C99 and a C program fills the specs; and the three coverage tables' parsers (tests/stream_cases.py,
tests/layout_cases.py, the prefixes of tests/test_sequence_cases.py) see none of the calls. What apply computes is held byte for byte to the mirror on the MI355X
(tests/test_shaping_gpu.py), what curl_host computes here (tests/test_shaping_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hnanosolver_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_shaping_create", "hns_shaping_destroy", "hns_shaping_set_stream", "hns_shaping_apply", "hns_shaping_curl_host")
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


def header():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    decl = re.search(r"^(?:int|void|hns_shaping\*)\s+%s\s*\(([^;]*)\);" % name, header(), re.M | re.S)
    assert decl, f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1  # one ctypes argument per parameter of the declaration


def test_the_structs_are_the_headers():
    h = header()
    body = re.search(r"typedef struct hns_turbulence_spec \{(.*?)\} hns_turbulence_spec;", h, re.S).group(1)
    members = re.findall(r"^\s*(?:int|float|unsigned int|const char\*)\s+(\w+)(?:\[3\])?;", body, re.M)
    assert members == [n for n, _ in _lib.hns_turbulence_spec._fields_] == ["amplitude", "frequency", "offset", "octaves", "lacunarity", "gain", "seed", "control",
                                                                              "control_lo", "control_hi"]
    assert C.sizeof(_lib.hns_turbulence_spec) == 56 and _lib.hns_turbulence_spec.control.offset == 40
    body = re.search(r"typedef struct hns_decay_spec \{(.*?)\} hns_decay_spec;", h, re.S).group(1)
    members = re.findall(r"^\s*(?:float|const char\*)\s+(\w+);", body, re.M)
    assert members == [n for n, _ in _lib.hns_decay_spec._fields_] == ["name", "rate", "target"] and C.sizeof(_lib.hns_decay_spec) == 16
    body = re.search(r"typedef struct hns_shaping_curl \{(.*?)\} hns_shaping_curl;", h, re.S).group(1)
    assert re.findall(r"^\s*float\s+(\w+)\[3\];", body, re.M) == [n for n, _ in _lib.hns_shaping_curl._fields_] == ["c"] and C.sizeof(_lib.hns_shaping_curl) == 12
    assert set(device.Shaping.TURBULENCE) == {n for n, _ in _lib.hns_turbulence_spec._fields_}


def test_header_states_the_arithmetic_line_by_line():
    h = header()
    comment = h[h.index("SHAPING A SIM"): h.index("typedef struct hns_shaping hns_shaping;")]
    for word in ("f_0 = frequency, f_o = f_(o-1) * lacunarity", "a_0 = 1.0f, a_o = a_(o-1) * gain", "kA = amplitude * dt", "inv = 1.0f / (control_hi - control_lo)",
                 "s_o = H(H(seed ^ 0x9E3779B9u) + o)", "r = 1.0f / (1.0f + rate * dt)", "q.c = f_o * (float)x.c; q.c = q.c + offset.c", "|q.c| >= 4194304.0f",
                 "I.c = Floor(q.c)", "t.c = q.c - (float)I.c", "H(H(H(s_o ^ (uint32)(I.x+a)) ^ (uint32)(I.y+b)) ^ (uint32)(I.z+e))", "(h >> 4m) & 15",
                 "(1,1,0), (-1,1,0), (1,-1,0), (-1,-1,0), (1,0,1), (-1,0,1), (1,0,-1), (-1,0,-1), (0,1,1), (0,-1,1), (0,1,-1), (0,-1,-1), (1,1,0), (-1,1,0), (0,-1,1), (0,-1,-1)",
                 "d_abe = (g.x * p.x + g.y * p.y) + g.z * p.z", "(((((6.0f * t - 15.0f) * t + 10.0f) * t) * t) * t", "b = t - 2.0f; b = b * t; b = b + 1.0f; e = 30.0f * t",
                 "d = v1 - v0; d = w * d; v0 + d", "dN_m/dx = u'(t.x) * L_yz(d_1be - d_0be) + L(g_abe.x)", "c_o.x = dN_2/dy - dN_1/dz; c_o.y = dN_0/dz - dN_2/dx; c_o.z = dN_1/dx - dN_0/dy",
                 "e = a_o * c_o.c; C.c = C.c + e", "BEFORE this call's decay", "w = c - control_lo", "w = fminf(fmaxf(w, 0.0f), 1.0f)", "a NaN c gives w = 0", "k = kA * w",
                 "e = k * C.c; v.c = v.c + e", "t = f - target; t = t * r; f = target + t", "launch range", "forgets", "hns_dist_*", "on average", "at the peak"):
        assert word in comment, word


def turbulence(**over):
    return device.Shaping.turbulence_spec({**dict(amplitude=2.0, frequency=0.125, octaves=2, seed=9), **over})


def decays(*rows):
    arr = (_lib.hns_decay_spec * max(1, len(rows)))()
    for d, (name, rate, target) in zip(arr, rows):
        d.name, d.rate, d.target = name, rate, target
    return arr


def test_every_refusal_of_a_number_comes_before_the_objects_are_looked_at():
    lib = _lib.load_library()
    nan, inf = float("nan"), float("inf")

    def call(dt=0.04, n_decays=None, rows=(), null_decays=False, no_turbulence=False, **over):
        tb, arr = turbulence(**over), decays(*rows)
        n = len(rows) if n_decays is None else n_decays
        return lambda: lib.hns_shaping_apply(None, None, dt, None if no_turbulence else C.byref(tb), None if null_decays else arr, n)

    rows = [
        (call(dt=nan), "dt"), (call(dt=inf), "dt"), (call(dt=-0.04), "dt"),
        (call(amplitude=nan), "amplitude"), (call(amplitude=inf), "amplitude"), (call(amplitude=-inf), "amplitude"),
        (call(frequency=0.0), "frequency"), (call(frequency=-0.5), "frequency"), (call(frequency=nan), "frequency"), (call(frequency=inf), "frequency"),
        (call(offset=(nan, 0, 0)), "offset"), (call(offset=(0, inf, 0)), "offset"), (call(offset=(0, 0, -inf)), "offset"),
        (call(octaves=0), "octaves"), (call(octaves=5), "octaves"), (call(octaves=-1), "octaves"),
        (call(lacunarity=0.99), "lacunarity"), (call(lacunarity=nan), "lacunarity"), (call(lacunarity=inf), "lacunarity"),
        (call(gain=-0.01), "gain"), (call(gain=1.01), "gain"), (call(gain=nan), "gain"),
        (call(control="density", control_lo=1.0, control_hi=1.0), "control_lo"), (call(control="density", control_lo=2.0, control_hi=1.0), "control_lo"),
        (call(control="density", control_lo=nan), "control_lo"), (call(control="density", control_hi=inf), "control_hi"), (call(control="density", control_lo=-inf), "control_lo"),
        (call(n_decays=-1), "n_decays"), (call(n_decays=9), "n_decays"), (call(n_decays=1, null_decays=True), "decays"),
        (call(rows=[(None, 1.0, 0.0)]), "name"), (call(rows=[(b"density", 1.0, 0.0), (None, 1.0, 0.0)]), "name"),
        (call(rows=[(b"density", nan, 0.0)]), "rate"), (call(rows=[(b"density", inf, 0.0)]), "rate"), (call(rows=[(b"density", -1.0, 0.0)]), "rate"),
        (call(rows=[(b"density", 1.0, nan)]), "target"), (call(rows=[(b"density", 1.0, inf)]), "target"),
        # a zero amplitude, or no turbulence at all, does not excuse a number
        (call(amplitude=0.0, octaves=5), "octaves"), (call(no_turbulence=True, dt=nan), "dt"), (call(no_turbulence=True, n_decays=9), "n_decays"),
        # every number in range (the ends of the ranges; control_lo / control_hi are not read without a control): the null object is what is refused
        (call(dt=0.0, amplitude=-3.0, octaves=1, lacunarity=1.0, gain=0.0, control_lo=nan, control_hi=nan), "null shaping"),
        (call(octaves=4, gain=1.0, control="density", control_lo=-1.0, control_hi=1.0, rows=[(b"density", 0.0, -2.0)] * 8), "null shaping"),
        (call(no_turbulence=True), "null shaping"),
    ]
    wrong = []
    for i, (fn, word) in enumerate(rows):
        lib.hns_set_option(b"rbgs", None)  # (a call that succeeds: whatever it leaves in hns_last_error(), the text read below is this row's)
        code, text = fn(), lib.hns_last_error().decode()
        if code != BAD or not text.startswith("hns_shaping_apply:") or word not in text:
            wrong.append(f"row {i} (expects {word!r}): got {code} {text!r}")
    assert not wrong, "\n".join(wrong)


def test_curl_host_and_set_stream_refuse_under_their_names():
    lib = _lib.load_library()
    out, good = _lib.hns_shaping_curl(), turbulence()
    for fn, who, word in ((lambda: lib.hns_shaping_curl_host(None, 0, 0, 0, C.byref(out)), "hns_shaping_curl_host:", "null spec"),
                          (lambda: lib.hns_shaping_curl_host(C.byref(good), 0, 0, 0, None), "hns_shaping_curl_host:", "null out"),
                          (lambda: lib.hns_shaping_curl_host(C.byref(turbulence(octaves=0)), 0, 0, 0, C.byref(out)), "hns_shaping_curl_host:", "octaves"),
                          (lambda: lib.hns_shaping_curl_host(C.byref(turbulence(frequency=0.0)), 0, 0, 0, C.byref(out)), "hns_shaping_curl_host:", "frequency"),
                          (lambda: lib.hns_shaping_set_stream(None, None), "hns_shaping_set_stream:", "null shaping")):
        lib.hns_set_option(b"rbgs", None)
        assert fn() == BAD
        text = lib.hns_last_error().decode()
        assert text.startswith(who) and word in text, text
    # control* is ignored: a spec apply would refuse evaluates
    assert lib.hns_shaping_curl_host(C.byref(turbulence(control="nope", control_lo=2.0, control_hi=1.0)), 1, 2, 3, C.byref(out)) == 0
    lib.hns_shaping_destroy(None)  # (a null object is allowed)


def test_create_without_a_device_is_no_device():
    lib = _lib.load_library()
    if lib.hns_device_count() == 0:  # (with a device, tests/test_shaping_gpu.py creates objects on it)
        err = C.c_int(0)
        assert not lib.hns_shaping_create(C.byref(err)) and err.value == _lib.HNS_ERR_NO_DEVICE
        text = lib.hns_last_error().decode()
        assert text.startswith("hns_shaping_create:") and "no HIP device" in text
        assert not lib.hns_shaping_create(None)  # (a null err is allowed)
        with pytest.raises(Exception, match="no HIP device"):
            device.Shaping()


def test_python_class_refuses_before_the_library_is_reached():
    with pytest.raises(ValueError, match="unknown turbulence keys"):
        device.Shaping.turbulence_spec({"amplitud": 1.0})
    with pytest.raises(ValueError, match="three components"):
        device.Shaping.turbulence_spec({"offset": (0.0, 1.0)})
    assert callable(device.Sim.shape) and callable(device.Shaping.apply) and callable(device.Shaping.close) and callable(device.shaping_curl_host)
    assert hasattr(device.Shaping, "__enter__") and hasattr(device.Shaping, "__exit__")


def test_header_is_plain_c99_and_a_c_program_fills_the_specs(tmp_path):
    src = tmp_path / "shaping_abi.c"
    src.write_text('#include "hns.h"\n#include <stdio.h>\n#include <string.h>\nint main(void) {\n'
                   '  hns_shaping_curl out = {{9.0f, 9.0f, 9.0f}};\n'
                   '  hns_turbulence_spec tb = {2.0f, 0.125f, {0.0f, -1.5f, 0.0f}, 2, 2.0f, 0.5f, 9u, NULL, 0.0f, 1.0f};\n'
                   '  hns_decay_spec dc[2] = {{"density", 0.5f, 0.0f}, {"temperature", 2.0f, 300.0f}};\n'
                   '  if (sizeof tb != 56 || sizeof dc[0] != 16 || sizeof out != 12) return 1;\n'
                   '  if (hns_shaping_curl_host(&tb, 8, 16, -24, &out) != HNS_OK || out.c[0] == 9.0f) return 2;\n'
                   '  if (hns_shaping_apply(NULL, NULL, 0.04f, &tb, dc, 2) != HNS_ERR_INVALID_ARGUMENT || !strstr(hns_last_error(), "null shaping")) return 3;\n'
                   '  tb.octaves = 5;\n'
                   '  if (hns_shaping_apply(NULL, NULL, 0.04f, &tb, dc, 2) != HNS_ERR_INVALID_ARGUMENT || !strstr(hns_last_error(), "octaves")) return 4;\n'
                   '  if (hns_shaping_set_stream(NULL, NULL) != HNS_ERR_INVALID_ARGUMENT) return 5;\n'
                   '  hns_shaping_destroy(NULL);\n  printf("shaping abi ok\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "shaping_abi")
    libdir = os.path.dirname(_lib.library_path())
    b = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lhns",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "shaping abi ok" in r.stdout, f"{r.returncode} {r.stdout} {r.stderr}"


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
    assert "hns_dev_temperature_buoyancy" in streamed and "hns_dev_temperature_buoyancy" in pointed  # (the parsers do see the header)
    for name in SYMBOLS:
        assert name not in streamed and name not in pointed and name.startswith(PREFIXES), name
        used = name in sequence_cases.RUNNER_SYMBOLS or any(name in o.symbols for o in sequence_cases.OPS.values())
        assert used != (name in sequence_cases.EXEMPT), name
        assert name not in stream_cases.CASES and name not in layout_cases.LAYOUT_CASES
