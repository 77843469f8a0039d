"""The owner of a pooled device block, the scratch of a call and the one way to lay slices over a block (hnanosolver_amd/csrc/hns_pool.hpp), and the two layouts under every
kernel (hns_internal.hpp: the sim's arena, the grid's tables), as a host-only program over a pool of its own (tests/cpp/pool_owner.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_scratch_carve_and_the_two_layouts_under_address_and_ub_sanitizers(tmp_path):
    """Every get matched by exactly one put on every path of the owner and the scratch, a put before the get that replaces it, nothing at all from an empty owner; carve at
    sizes 0, 1, 255, 256, 257 and a slice in units; the sim arena's and the grid tables' offsets against literals worked by hand. Built with -fsanitize=address,undefined
    like tests/test_sor_schedule.py's program, and run on its own with LeakSanitizer on (nothing of it is loaded into Python)."""
    rocm_inc = "/opt/rocm/include"
    assert os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")), "hns_internal.hpp includes the HIP headers: they belong to the build environment"
    exe = str(tmp_path / "pool_owner")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hnanosolver_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "pool_owner.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "pool_owner OK" in r.stdout, r.stdout + r.stderr[-3000:]
