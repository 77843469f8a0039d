"""What lets the look-ahead form of advect_scalars run four workgroups per CU (eight waves per SIMD), pinned from the device listing that
csrc/Makefile's `%.s` rule writes, read as tests/test_kernel_resources.py reads it.

k_advect_scalars_n<false, true>: a 512-thread workgroup has a quarter of a CU when it takes at most 64 registers (VGPRs and AGPRs share one
file, so no AGPR) and at most 160 KB / 4 = 40,960 B of LDS, and it must get there without a spill (an SGPR spilled into a VGPR's lanes counts:
it is how the kernel reached a 65th register) or scratch.
k_advect_vector_n and k_advect_vector_n<true>: their velocity box holds x and y in interleaved rows, two planes where it took three; the LDS of
either lies BELOW what it compiled to before the interleaved layout (29,208 and 38,808 B, from the listing of the commit before it)."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

LOOKAHEAD = "18k_advect_scalars_nILb0ELb1EEE"
# mangled-name fragment: (kernel, LDS bytes of the three-plane box)
VECTOR_LDS_BEFORE = {
    "17k_advect_vector_nENS": ("k_advect_vector_n", 29208),
    "17k_advect_vector_nILb1EEE": ("k_advect_vector_n<true>", 38808),
}


@pytest.fixture(scope="module")
def advect_kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_advect.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def only(kernels, fragment):
    found = [m for name, m in kernels.items() if fragment in name]
    assert len(found) == 1, f"{len(found)} kernels match {fragment}"
    return found[0]


def test_lookahead_form_fits_four_workgroups_per_cu(advect_kernels):
    m = only(advect_kernels, LOOKAHEAD)
    print(f"k_advect_scalars_n<false, true>: vgpr {m['vgpr_count']}, agpr {m['agpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_count"] <= 64, f"{m['vgpr_count']} VGPRs"
    assert m["agpr_count"] == 0, f"{m['agpr_count']} AGPRs"
    assert m["group_segment_fixed_size"] <= 40960, f"{m['group_segment_fixed_size']} B of LDS"
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, "spills"
    assert m["private_segment_fixed_size"] == 0, "uses scratch"


@pytest.mark.parametrize("fragment", sorted(VECTOR_LDS_BEFORE))
def test_vector_kernels_hold_a_two_plane_box(advect_kernels, fragment):
    kernel, before = VECTOR_LDS_BEFORE[fragment]
    m = only(advect_kernels, fragment)
    print(f"{kernel}: lds {m['group_segment_fixed_size']} (< {before})")
    assert m["group_segment_fixed_size"] < before, f"{kernel}: {m['group_segment_fixed_size']} B of LDS, {before} with three planes"
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, f"{kernel} spills"
