"""Registers, LDS and spills of the three 32-bit addressed advection kernels with a collision SDF (hns_advect.hip), read from the device listing as
tests/test_kernel_resources.py reads them for the kernels it pins.

Bounds, from the first accepted build:
  k_advect_vector_n<true>               58 VGPRs -> the 64-register granule (amdgpu_waves_per_eu(8, 8)): eight waves per SIMD = four 512-thread workgroups per CU,
                                         and 38,808 B of LDS (velocity box, SDF box with rows 24 apart, tables): four of them are 155 KB of gfx950's 160 KB
  k_advect_scalars_n<false,false,true>  62 VGPRs -> the 64-register granule, 12,408 B of LDS (two float boxes, the SDF box, tables): registers bound it, four workgroups per CU
  k_advect_scalars_n<true,false,true>   80 VGPRs -> the 80-register line: six waves per SIMD = three workgroups per CU, and 46,560 B of LDS (velocity box, two float boxes,
                                         the 16-byte box, the SDF box, the back positions, tables): three of them are 140 KB
A kernel may not pass its granule, its LDS may not grow, nothing spills or uses scratch, and each exists exactly once."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound, LDS bytes bound)
BOUNDS = {
    "17k_advect_vector_nILb1EE": ("k_advect_vector_n<true>", 64, 38808),
    "18k_advect_scalars_nILb0ELb0ELb1EE": ("k_advect_scalars_n<false, false, true>", 64, 12408),
    "18k_advect_scalars_nILb1ELb0ELb1EE": ("k_advect_scalars_n<true, false, true>", 80, 46560),
}


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
def test_collision_advection_kernel_resources(advect_listing, fragment):
    kernel, vgpr_bound, lds_bound = BOUNDS[fragment]
    found = [m for name, m in advect_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"


def test_no_other_collision_instantiation(advect_listing):
    """the look-ahead form has no collision instantiation (static_assert), and the no-collision kernels keep their names"""
    names = [n for n in advect_listing if "18k_advect_scalars_nI" in n or "17k_advect_vector_n" in n]
    assert len(names) == 7, names
