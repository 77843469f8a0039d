"""Registers, LDS and spills of the two diagnostics kernels, read as tests/test_kernel_resources.py reads the advection kernels': from the metadata at
the end of the device listing that csrc/Makefile's `%.s` rule writes.

Bounds (what the first build showed): a kernel's VGPR count may not pass the allocation granule (8) it sits in -- k_field_stats 90 of 96 (eight velocity
loads in flight are 24 registers, three f64 accumulator pairs 12), k_residual 55 of 56 -- its LDS may not grow (k_residual: the 896-float tile of p plus
512 floats of c = 5,632 B), and nothing spills."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound, LDS bytes bound)
BOUNDS = {
    "13k_field_statsE": ("k_field_stats", 96, 0),
    "10k_residualE": ("k_residual", 56, 5632),
}


@pytest.fixture(scope="module")
def diagnostics_kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_diagnostics.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_diagnostics_kernel_resources(diagnostics_kernels, fragment):
    kernel, vgpr_bound, lds_bound = BOUNDS[fragment]
    found = [m for name, m in diagnostics_kernels.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"
