"""Registers, LDS and spills of the kernels of hns_rasterize.hip (k_splat_radial<1 | 4 | 16 | 64>), read from the device listing as tests/test_splat_resources.py reads
them for hns_splat.hip: every kernel of the file is listed, nothing spills, nothing uses scratch, nothing uses LDS, and the vector registers are the ones the first
accepted build used (DESIGN.md section 4 records them): at most 64, so that eight waves a SIMD fit and the adds in flight are what bounds the kernel."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, vector registers)
KERNELS = {
    "14k_splat_radialILi1E": ("k_splat_radial<1>", 22),
    "14k_splat_radialILi4E": ("k_splat_radial<4>", 32),
    "14k_splat_radialILi16E": ("k_splat_radial<16>", 34),
    "14k_splat_radialILi64E": ("k_splat_radial<64>", 32),
}


@pytest.fixture(scope="module")
def listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_rasterize.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(listing):
    assert len(listing) == len(KERNELS)
    for name in listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_rasterize.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_radial_kernel_resources(listing, fragment):
    kernel, vgprs = KERNELS[fragment]
    found = [m for name, m in listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == 0, f"{kernel} uses LDS"
    assert m["vgpr_count"] == vgprs, f"{kernel}: {m['vgpr_count']} vector registers, {vgprs} recorded"
