"""Registers, LDS and spills of the kernels of hns_splat.hip (k_splat_points, k_splat_finish<1 .. 4>), read from the device listing as tests/test_points_resources.py
reads them for the kernels of hns_points.hip: nothing spills, nothing uses scratch. The register counts of the first accepted build are recorded in DESIGN.md (section 4);
they are not gated here beyond that."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: kernel
KERNELS = {
    "14k_splat_pointsILb0E": "k_splat_points<false>",
    "14k_splat_finishILi1E": "k_splat_finish<1>",
    "14k_splat_finishILi2E": "k_splat_finish<2>",
    "14k_splat_finishILi3E": "k_splat_finish<3>",
    "14k_splat_finishILi4E": "k_splat_finish<4>",
}


@pytest.fixture(scope="module")
def splat_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_splat.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(splat_listing):
    for name in splat_listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_splat.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_splat_kernel_resources(splat_listing, fragment):
    kernel = KERNELS[fragment]
    found = [m for name, m in splat_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
