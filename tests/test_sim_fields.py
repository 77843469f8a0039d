"""The host preamble of a sim call (hnanosolver_amd/csrc/hns_simcall.hpp): the one resolver of a named float-field list, check_sim -- the lent-sim refusal included, which
no call through the ABI reaches --, sim_grid and the row-move and capacity checks, as a host-only program over shell objects (tests/cpp/sim_fields.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_lists_check_sim_and_the_row_checks_under_address_and_ub_sanitizers(tmp_path):
    """sim_fields: indices in list order, n = -1 with and without the flag, n below it, a null list, a null name, an unknown name, collision_sdf with and without a
    reason, a duplicate through a plain list and through a struct array (the same code, the same text up to the list's label), `which` empty after every refusal, every
    refusal HNS_ERR_INVALID_ARGUMENT under "<who>: ". check_sim: a cached and a lent sim, null with and without a device. check_rows at row_bytes 0, 2, 4, 6, 64, 68, null
    and equal pointers, no rows, no run; check_capacity at the capacity and one above. Built with -fsanitize=address,undefined like tests/test_pool_owner.py's program, and
    run on its own (nothing of it is loaded into Python)."""
    rocm_inc = "/opt/rocm/include"
    assert os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")), "hns_internal.hpp includes the HIP headers: they belong to the build environment"
    exe = str(tmp_path / "sim_fields")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hnanosolver_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "sim_fields.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "sim_fields OK" in r.stdout, r.stdout + r.stderr[-3000:]
