"""hns_diffusion_* without a GPU: exported, declared and bound; the three structs are the header's; the header states the arithmetic line by line; create without a
device gives HNS_ERR_NO_DEVICE; every refusal of a number or of a host struct returns HNS_ERR_INVALID_ARGUMENT with the call and the argument in the message before any
object is looked at (null objects serve); the header compiles as strict C99 and a C program fills the specs and calls schedule_host; and the three coverage tables'
parsers (tests/stream_cases.py, tests/layout_cases.py, the prefixes of tests/test_sequence_cases.py) see none of the calls. What apply computes is held word for word to
the mirror on the MI355X (tests/test_diffusion_gpu.py), what schedule_host computes here (tests/test_diffusion_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hnanosolver_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_diffusion_create", "hns_diffusion_destroy", "hns_diffusion_set_stream", "hns_diffusion_apply", "hns_diffusion_schedule_host")
BAD = _lib.HNS_ERR_INVALID_ARGUMENT


def header():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    decl = re.search(r"^(?:int|void|hns_diffusion\*)\s+%s\s*\(([^;]*)\);" % name, header(), re.M | re.S)
    assert decl, f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1  # one ctypes argument per parameter of the declaration


def test_the_structs_are_the_headers():
    h = header()
    body = re.search(r"typedef struct hns_diffusion_term \{(.*?)\} hns_diffusion_term;", h, re.S).group(1)
    members = re.findall(r"^\s*(?:float|const char\*)\s+(\w+);", body, re.M)
    assert members == [n for n, _ in _lib.hns_diffusion_term._fields_] == ["name", "coefficient"] and C.sizeof(_lib.hns_diffusion_term) == 16
    body = re.search(r"typedef struct hns_diffusion_spec \{(.*?)\} hns_diffusion_spec;", h, re.S).group(1)
    members = re.findall(r"^\s*(?:int|float)\s+(\w+);", body, re.M)
    assert members == [n for n, _ in _lib.hns_diffusion_spec._fields_] == ["iterations", "method", "viscosity", "collide", "threshold"]
    assert C.sizeof(_lib.hns_diffusion_spec) == 20
    body = re.search(r"typedef struct hns_diffusion_schedule \{(.*?)\} hns_diffusion_schedule;", h, re.S).group(1)
    members = re.findall(r"^\s*float\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert members == [("a", ""), ("r", "7"), ("rho", ""), ("omega", "256")] and [n for n, _ in members] == [n for n, _ in _lib.hns_diffusion_schedule._fields_]
    assert C.sizeof(_lib.hns_diffusion_schedule) == 4 * (1 + 7 + 1 + 256) and _lib.hns_diffusion_schedule.omega.offset == 36
    assert device.Diffusion.METHODS == {"jacobi": 0, "chebyshev": 1}


def test_header_states_the_arithmetic_line_by_line():
    h = header()
    comment = h[h.index("DIFFUSING A SIM"): h.index("typedef struct hns_diffusion hns_diffusion;")]
    for word in ("(I - a L) x = b", "a = coefficient * dt / voxel_size^2", "7-point Laplacian over the UNKNOWNS",
                 "SOLID iff collide != 0, its leaf exists and collision_sdf < threshold", "a NaN is not solid", "UNKNOWN iff its leaf exists", "it is never written",
                 "+x, -x, +y, -y, +z, -z", "OPEN: the neighbour is an unknown", "WALL: the neighbour is solid", "zero-flux", "no-slip wall at rest",
                 "m = open faces for a float field", "m = open + wall faces", "h2 = voxel_size * voxel_size; a = coefficient * dt; a = a / h2",
                 "e = a * (float)m; den = 1.0f + e; r_m = 1.0f / den", "s = 6.0f * a; den = 1.0f + s; rho = s / den; q = rho * rho", "w_2 = 1.0f / (1.0f - q * 0.5f)",
                 "h = q * 0.5f; d = 1.0f - h; w_2 = 1.0f / d", "w_(k+1) = 1.0f / (1.0f - (q * 0.25f) * w_k)", "c = q * 0.25f; e = c * w_k; d = 1.0f - e; w_(k+1) = 1.0f / d",
                 "no division on the device", "x^0 = b; S = +0.0f", "S = S + x^(k-1)[neighbour]; t = a * S; t = b + t; j = t * r_m", "Jacobi (method 0): x^k = j",
                 "x^1 = j; for k >= 2: d = j - x^(k-2); d = w_k * d; x^k = x^(k-2) + d", "x^k may be written over x^(k-2)", "There are no atomics",
                 "contracts the max-norm error by rho", "[min b, max b]", "2 sigma^k / (1 + sigma^(2k))", "sigma = rho / (1 + sqrt(1 - rho^2))", "loses that monotonicity",
                 "conserves the sum", "the wall takes momentum", "a term whose a is +0", "neither read nor written", "forgets", "launch range", "two iterates beside b",
                 "from the pool", "no result depends on what that memory held", "omega[k-1] = w_k", "hns_dist_*"):
        assert word in comment, word


def spec(**over):
    return _lib.hns_diffusion_spec(*[{**dict(iterations=8, method=0, viscosity=0.01, collide=0, threshold=0.0), **over}[k] for k, _ in _lib.hns_diffusion_spec._fields_])


def terms(*rows):
    arr = (_lib.hns_diffusion_term * max(1, len(rows)))()
    for t, (name, coefficient) in zip(arr, rows):
        t.name, t.coefficient = name, coefficient
    return arr


def test_every_refusal_of_a_number_comes_before_the_objects_are_looked_at():
    lib = _lib.load_library()
    nan, inf = float("nan"), float("inf")

    def call(dt=0.04, vs=1.0 / 32, n_terms=None, rows=(), null_terms=False, null_spec=False, **over):
        sp, arr = spec(**over), terms(*rows)
        n = len(rows) if n_terms is None else n_terms
        return lambda: lib.hns_diffusion_apply(None, None, dt, vs, None if null_spec else C.byref(sp), None if null_terms else arr, n)

    rows = [
        (call(dt=nan), "dt"), (call(dt=inf), "dt"), (call(dt=-0.04), "dt"),
        (call(vs=0.0), "voxel_size"), (call(vs=-1.0), "voxel_size"), (call(vs=nan), "voxel_size"), (call(vs=inf), "voxel_size"),
        (call(null_spec=True), "null spec"),
        (call(iterations=0), "iterations"), (call(iterations=257), "iterations"), (call(iterations=-1), "iterations"),
        (call(method=-1), "method"), (call(method=2), "method"),
        (call(viscosity=nan), "viscosity"), (call(viscosity=inf), "viscosity"), (call(viscosity=-0.5), "viscosity"),
        (call(viscosity=1e30, vs=1e-10), "not finite"), (call(viscosity=3e38, dt=0.2, vs=1.0), "not finite"),  # a = inf; a finite and 6 a = inf
        (call(viscosity=1.0, vs=1e-30), "not finite"),  # voxel_size^2 rounds to 0
        (call(collide=1, threshold=nan), "threshold"), (call(collide=1, threshold=inf), "threshold"),
        (call(n_terms=-1), "n_terms"), (call(n_terms=9), "n_terms"), (call(n_terms=1, null_terms=True), "terms"),
        (call(rows=[(None, 1.0)]), "name"), (call(rows=[(b"density", 1.0), (None, 1.0)]), "name"),
        (call(rows=[(b"density", nan)]), "coefficient"), (call(rows=[(b"density", inf)]), "coefficient"), (call(rows=[(b"density", -1.0)]), "coefficient"),
        (call(rows=[(b"density", 1e30)], vs=1e-10), "not finite"),
        # a zero dt (every a is 0: nothing would be launched) does not excuse a number
        (call(dt=0.0, iterations=0), "iterations"), (call(dt=0.0, rows=[(b"density", -1.0)]), "coefficient"),
        # every number in range (the ends of the ranges; the threshold is not read without collide): the null object is what is refused
        (call(dt=0.0, iterations=1, viscosity=0.0, threshold=nan), "null diffusion"),
        (call(iterations=256, method=1, collide=1, threshold=-3.0, rows=[(b"density", 0.0)] * 8), "null diffusion"),
    ]
    wrong = []
    for i, (fn, word) in enumerate(rows):
        lib.hns_set_option(b"rbgs", None)  # (a call that succeeds: whatever it leaves in hns_last_error(), the text read below is this row's)
        code, text = fn(), lib.hns_last_error().decode()
        if code != BAD or not text.startswith("hns_diffusion_apply:") or word not in text:
            wrong.append(f"row {i} (expects {word!r}): got {code} {text!r}")
    assert not wrong, "\n".join(wrong)


def test_schedule_host_and_set_stream_refuse_under_their_names():
    lib = _lib.load_library()
    out = _lib.hns_diffusion_schedule()
    nan, inf = float("nan"), float("inf")
    for fn, who, word in ((lambda: lib.hns_diffusion_schedule_host(1.0, 0.04, 1.0, 8, None), "hns_diffusion_schedule_host:", "null out"),
                          (lambda: lib.hns_diffusion_schedule_host(nan, 0.04, 1.0, 8, C.byref(out)), "hns_diffusion_schedule_host:", "coefficient"),
                          (lambda: lib.hns_diffusion_schedule_host(-1.0, 0.04, 1.0, 8, C.byref(out)), "hns_diffusion_schedule_host:", "coefficient"),
                          (lambda: lib.hns_diffusion_schedule_host(1.0, -0.04, 1.0, 8, C.byref(out)), "hns_diffusion_schedule_host:", "dt"),
                          (lambda: lib.hns_diffusion_schedule_host(1.0, inf, 1.0, 8, C.byref(out)), "hns_diffusion_schedule_host:", "dt"),
                          (lambda: lib.hns_diffusion_schedule_host(1.0, 0.04, 0.0, 8, C.byref(out)), "hns_diffusion_schedule_host:", "voxel_size"),
                          (lambda: lib.hns_diffusion_schedule_host(1.0, 0.04, 1.0, 0, C.byref(out)), "hns_diffusion_schedule_host:", "iterations"),
                          (lambda: lib.hns_diffusion_schedule_host(1.0, 0.04, 1.0, 257, C.byref(out)), "hns_diffusion_schedule_host:", "iterations"),
                          (lambda: lib.hns_diffusion_schedule_host(1e30, 1.0, 1e-10, 8, C.byref(out)), "hns_diffusion_schedule_host:", "not finite"),
                          (lambda: lib.hns_diffusion_set_stream(None, None), "hns_diffusion_set_stream:", "null diffusion")):
        lib.hns_set_option(b"rbgs", None)
        assert fn() == BAD
        text = lib.hns_last_error().decode()
        assert text.startswith(who) and word in text, text
    assert lib.hns_diffusion_schedule_host(0.0, 0.0, 1.0, 256, C.byref(out)) == 0 and out.a == 0 and out.rho == 0 and list(out.r) == [1.0] * 7 and out.omega[255] == 1.0
    lib.hns_diffusion_destroy(None)  # (a null object is allowed)


def test_create_without_a_device_is_no_device():
    lib = _lib.load_library()
    if lib.hns_device_count() == 0:  # (with a device, tests/test_diffusion_gpu.py creates objects on it)
        err = C.c_int(0)
        assert not lib.hns_diffusion_create(C.byref(err)) and err.value == _lib.HNS_ERR_NO_DEVICE
        text = lib.hns_last_error().decode()
        assert text.startswith("hns_diffusion_create:") and "no HIP device" in text
        assert not lib.hns_diffusion_create(None)  # (a null err is allowed)
        with pytest.raises(Exception, match="no HIP device"):
            device.Diffusion()


def test_python_class_refuses_before_the_library_is_reached():
    with pytest.raises(ValueError, match="unknown method"):
        device.Diffusion.spec(method="gauss-seidel")

    class NoSim:
        names = ["density"]
        _ptr = None

    shell = device.Diffusion.__new__(device.Diffusion)  # (no device here: the checks in front of the library are what is tested)
    shell._ptr = 1
    try:
        with pytest.raises(ValueError, match="unknown method"):
            shell.apply(NoSim(), 0.04, 1.0, {"density": 1.0}, method="sor")
        with pytest.raises(ValueError, match="unknown fields"):
            shell.apply(NoSim(), 0.04, 1.0, {"densty": 1.0})
    finally:
        shell._ptr = 0
    assert callable(device.Sim.diffuse) and callable(device.Diffusion.apply) and callable(device.Diffusion.close) and callable(device.diffusion_schedule_host)
    assert hasattr(device.Diffusion, "__enter__") and hasattr(device.Diffusion, "__exit__")


def test_header_is_plain_c99_and_a_c_program_fills_the_specs(tmp_path):
    src = tmp_path / "diffusion_abi.c"
    src.write_text('#include "hns.h"\n#include <stdio.h>\n#include <string.h>\nint main(void) {\n'
                   '  hns_diffusion_schedule out;\n'
                   '  hns_diffusion_spec sp = {8, 1, 0.01f, 1, 0.0f};\n'
                   '  hns_diffusion_term tm[2] = {{"density", 0.5f}, {"temperature", 2.0f}};\n'
                   '  if (sizeof sp != 20 || sizeof tm[0] != 16 || sizeof out != 1060) return 1;\n'
                   '  if (hns_diffusion_schedule_host(0.5f, 1.0f, 1.0f, 3, &out) != HNS_OK || out.a != 0.5f || out.r[2] != 0.5f || out.rho != 0.75f) return 2;\n'
                   '  if (out.omega[0] != 1.0f || !(out.omega[1] > 1.0f) || !(out.omega[2] > 1.0f) || out.omega[3] != 0.0f) return 3;\n'
                   '  if (hns_diffusion_apply(NULL, NULL, 0.04f, 1.0f, &sp, tm, 2) != HNS_ERR_INVALID_ARGUMENT || !strstr(hns_last_error(), "null diffusion")) return 4;\n'
                   '  sp.iterations = 257;\n'
                   '  if (hns_diffusion_apply(NULL, NULL, 0.04f, 1.0f, &sp, tm, 2) != HNS_ERR_INVALID_ARGUMENT || !strstr(hns_last_error(), "iterations")) return 5;\n'
                   '  if (hns_diffusion_set_stream(NULL, NULL) != HNS_ERR_INVALID_ARGUMENT) return 6;\n'
                   '  hns_diffusion_destroy(NULL);\n  printf("diffusion abi ok\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "diffusion_abi")
    libdir = os.path.dirname(_lib.library_path())
    b = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lhns",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "diffusion abi ok" in r.stdout, f"{r.returncode} {r.stdout} {r.stderr}"


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
