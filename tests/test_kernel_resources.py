"""The occupancy facts that DESIGN.md 4 and 7 build on, pinned: registers, LDS and spills of the five 32-bit addressed advection
kernels, read from the metadata at the end of the device listing that csrc/Makefile's `%.s` rule writes (the flags of the build).

Bounds: a kernel's VGPR count may not pass the allocation granule (8) it sits in, its LDS may not grow, and nothing spills.
k_advect_scalars_n<true> (q4) at 80 registers and <false, true> (look-ahead) at 72 / 43,468 B are six waves per SIMD = three
workgroups per CU: one granule or one more LDS allocation step over it is a workgroup less (hns_advect.hip)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hnanosolver_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")

# mangled-name fragment: (kernel, VGPR bound, LDS bytes bound)
BOUNDS = {
    "17k_advect_vector_nE": ("k_advect_vector_n", 64, 29212),
    "17k_advect_scalar_nE": ("k_advect_scalar_n", 56, 3996),
    "18k_advect_scalars_nILb0ELb0EE": ("k_advect_scalars_n<false, false>", 64, 8524),
    "18k_advect_scalars_nILb0ELb1EE": ("k_advect_scalars_n<false, true>", 72, 43468),
    "18k_advect_scalars_nILb1ELb0EE": ("k_advect_scalars_n<true, false>", 80, 36528),
}


def kernel_metadata(listing):
    """{mangled kernel name: {metadata key: int}} of the amdhsa.kernels list of a device listing"""
    out = {}
    for block in re.split(r"\n  - (?=\.)", listing[listing.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


@pytest.fixture(scope="module")
def advect_kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_advect.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_narrow_advection_kernel_resources(advect_kernels, fragment):
    kernel, vgpr_bound, lds_bound = BOUNDS[fragment]
    found = [m for name, m in advect_kernels.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']} (<= {lds_bound})")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
    assert m["group_segment_fixed_size"] <= lds_bound, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, bound {lds_bound}"
