"""Registers, LDS and spills of the kernels of hns_neighbours.hip (k_cell_table, k_neighbours<4 | 16 | 32, ranked | original>), read from the device listing as
tests/test_splat_resources.py reads them for the kernels of hns_splat.hip: every kernel of the file is named here, nothing spills, nothing uses scratch. The register
counts of the first accepted build are recorded in DESIGN.md (section 4); they are not gated here beyond that."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: kernel
KERNELS = {
    "12k_cell_table": "k_cell_table",
    "12k_neighboursILi4ELb1E": "k_neighbours<4, ranked>",
    "12k_neighboursILi4ELb0E": "k_neighbours<4, original>",
    "12k_neighboursILi16ELb1E": "k_neighbours<16, ranked>",
    "12k_neighboursILi16ELb0E": "k_neighbours<16, original>",
    "12k_neighboursILi32ELb1E": "k_neighbours<32, ranked>",
    "12k_neighboursILi32ELb0E": "k_neighbours<32, original>",
}


@pytest.fixture(scope="module")
def neighbours_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_neighbours.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(neighbours_listing):
    assert len(neighbours_listing) == len(KERNELS)
    for name in neighbours_listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_neighbours.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_neighbour_kernel_resources(neighbours_listing, fragment):
    kernel = KERNELS[fragment]
    found = [m for name, m in neighbours_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
