"""Registers, LDS and spills of the kernels of hns_splat_binned.hip, read from the kernel metadata of the device listing as tests/test_point_order_resources.py reads them
for hns_pointorder.hip: every kernel of the file is listed, nothing spills, nothing uses scratch, and the LDS of each kernel is at or below the figure its static_assert
states in the source. The register counts are printed and not gated."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

LEAF_LDS = 17 * 1024  # static_assert(kLdsLeaf <= 17 * 1024): 512 x 4 int64 sums, the mask copy, the source ranges

# mangled-name fragment: (kernel, LDS bytes its static_assert allows)
KERNELS = {
    "15k_binned_pointsILb0": ("k_binned_points<false>", 0),
    "15k_binned_pointsILb1": ("k_binned_points<true>", 0),
    "13k_binned_leafILi0E": ("k_binned_leaf<0>", LEAF_LDS),
    "13k_binned_leafILi1E": ("k_binned_leaf<1>", LEAF_LDS),
    "13k_binned_leafILi4E": ("k_binned_leaf<4>", LEAF_LDS),
    "13k_binned_leafILi16E": ("k_binned_leaf<16>", LEAF_LDS),
    "13k_binned_leafILi64E": ("k_binned_leaf<64>", LEAF_LDS),
}


@pytest.fixture(scope="module")
def binned_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_splat_binned.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(binned_listing):
    assert len(binned_listing) == len(KERNELS)
    for name in binned_listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_splat_binned.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_splat_binned_kernel_resources(binned_listing, fragment):
    kernel, lds = KERNELS[fragment]
    found = [m for name, m in binned_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] <= lds, f"{kernel} uses {m['group_segment_fixed_size']} bytes of LDS, above the {lds} its static_assert states"
