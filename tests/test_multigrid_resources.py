"""Registers, LDS and spills of the four multigrid kernels (hns_multigrid.hip), read as tests/test_kernel_resources.py reads the advection kernels': from the metadata
at the end of the device listing that csrc/Makefile's `%.s` rule writes.

Bounds (what the first build showed): a kernel's VGPR count may not pass the allocation granule (8) it sits in -- k_mg_masks 14 of 16, k_mg_color 13 of 16,
k_mg_restrict 32 of 32, k_mg_prolong 32 of 32 --, its LDS may not grow (k_mg_color: the 27 neighbour ids; k_mg_restrict: eight 896-float tiles of p, one per child leaf =
28,672 B; k_mg_prolong: the 6^3 coarse voxels around an octant = 864 B), and nothing spills or uses scratch."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound, LDS bytes bound)
BOUNDS = {
    "10k_mg_masksE": ("k_mg_masks", 16, 0),
    "10k_mg_colorE": ("k_mg_color", 16, 108),
    "13k_mg_restrictE": ("k_mg_restrict", 32, 28672),
    "12k_mg_prolongE": ("k_mg_prolong", 32, 864),
}


@pytest.fixture(scope="module")
def multigrid_kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_multigrid.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_multigrid_kernel_resources(multigrid_kernels, fragment):
    kernel, vgpr_bound, lds_bound = BOUNDS[fragment]
    found = [m for name, m in multigrid_kernels.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"
