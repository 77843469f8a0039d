"""Registers, LDS and spills of k_advect_scalar_multi_n (hns_advect.hip), read from the device listing as tests/test_kernel_resources.py reads them for the
five kernels it pins.

Bounds: the first accepted build has 62 VGPRs (amdgpu_waves_per_eu(8, 8)) -- the 64-register allocation granule, eight waves per SIMD, four 512-thread workgroups per CU --
and 7,576 B of LDS (the leaf tables and two clamp tiles). The kernel may not pass that granule, its LDS may not grow, and nothing spills or uses scratch."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound, LDS bytes bound)
BOUNDS = {"23k_advect_scalar_multi_n": ("k_advect_scalar_multi_n", 64, 7576)}


@pytest.fixture(scope="module")
def advect_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_advect.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_multi_field_advection_kernel_resources(advect_listing, fragment):
    kernel, vgpr_bound, lds_bound = BOUNDS[fragment]
    found = [m for name, m in advect_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"
