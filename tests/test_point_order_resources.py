"""Registers, LDS and spills of the kernels of hns_pointorder.hip, read from the kernel metadata of the device listing as tests/test_seed_resources.py reads them for
hns_seed.hip: every kernel of the file is listed, nothing spills, nothing uses scratch, and the LDS of each kernel is at or below the figure its static_assert states in
the source. The register counts of the first accepted build are recorded in DESIGN.md (section 4); they are printed here and not gated."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, LDS bytes its static_assert allows)
KERNELS = {
    "12k_order_keys": ("k_order_keys", 1024),
    "12k_order_hist": ("k_order_hist", 1024),
    "14k_order_totals": ("k_order_totals", 16),
    "12k_order_scan": ("k_order_scan", 16),
    "15k_order_scatterILb0": ("k_order_scatter<false>", 22 * 1024),
    "15k_order_scatterILb1": ("k_order_scatter<true>", 22 * 1024),
    "14k_order_ranges": ("k_order_ranges", 0),
    "12k_order_rowsILb0": ("k_order_rows<false>", 0),
    "12k_order_rowsILb1": ("k_order_rows<true>", 0),
}


@pytest.fixture(scope="module")
def order_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_pointorder.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(order_listing):
    assert len(order_listing) == len(KERNELS)
    for name in order_listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_pointorder.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_point_order_kernel_resources(order_listing, fragment):
    kernel, lds = KERNELS[fragment]
    found = [m for name, m in order_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] <= lds, f"{kernel} uses {m['group_segment_fixed_size']} bytes of LDS, above the {lds} its static_assert states"
