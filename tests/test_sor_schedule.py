"""The pressure loop's launch schedule (hnanosolver_amd/csrc/hns_internal.hpp: hns::sor_schedule) as a host-only program: the value hns_rbgs_iterate walks and
hns_grid_rbgs_plan describes, against the two loops it replaced and a hand-written table (tests/cpp/sor_schedule.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_matches_the_loops_it_replaced_under_address_and_ub_sanitizers(tmp_path):
    """lb in {0, 1, 2}, k_max in {2, 4} (4 with one-leaf blocks only), iterations 0 .. 64: steps in order, kernel launches and iterations per launch; built with
    -fsanitize=address,undefined like tests/test_abi.py's host program, and run on its own (nothing of it is loaded into Python)."""
    rocm_inc = "/opt/rocm/include"
    assert os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")), "hns_internal.hpp includes the HIP headers: they belong to the build environment"
    exe = str(tmp_path / "sor_schedule")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hnanosolver_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "sor_schedule.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "sor_schedule OK (260 cases)" in r.stdout, r.stdout + r.stderr[-3000:]
