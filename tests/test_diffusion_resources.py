"""Registers, LDS and spills of the kernels of hns_diffusion.hip, read from the device listing as tests/test_shaping_resources.py reads them for hns_shaping.hip.

Bounds: nothing spills, nothing uses scratch, and no kernel's VGPR count may pass the allocation granule (8 registers) the first accepted build sits in. That build has:
k_diffuse<Chebyshev, velocity> = <false, false> 23 VGPRs (bound 24), <true, false> 24 (24), <false, true> 40 (40), <true, true> 42 (48) -- every form far below the 64 at
which a 512-thread workgroup's eight waves stop fitting four times on a CU, so the file is built WITH the SLP vectoriser (the Makefile says so); k_diffuse_faces 10 (16),
k_diffuse_copy 8 (8). LDS: k_diffuse holds two tiles of 896 floats (a leaf's 512 values and the 384 of its neighbours' face layers; two, so that a field costs one
barrier) and the 27 neighbour ids, 2 * 896 * 4 + 27 * 4 = 7,276 bytes; k_diffuse_faces one tile of 896 class bytes and the ids, 896 + 108 = 1,004; k_diffuse_copy none."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

TILE = 512 + 6 * 64
# mangled-name fragment: (kernel, VGPR bound, LDS bytes)
BOUNDS = {
    "9k_diffuseILb0ELb0EE": ("k_diffuse<false, false>", 24, 2 * TILE * 4 + 27 * 4),
    "9k_diffuseILb1ELb0EE": ("k_diffuse<true, false>", 24, 2 * TILE * 4 + 27 * 4),
    "9k_diffuseILb0ELb1EE": ("k_diffuse<false, true>", 40, 2 * TILE * 4 + 27 * 4),
    "9k_diffuseILb1ELb1EE": ("k_diffuse<true, true>", 48, 2 * TILE * 4 + 27 * 4),
    "15k_diffuse_faces": ("k_diffuse_faces", 16, TILE + 27 * 4),
    "14k_diffuse_copy": ("k_diffuse_copy", 8, 0),
}


@pytest.fixture(scope="module")
def diffusion_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_diffusion.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_bounded(diffusion_listing):
    assert len(diffusion_listing) == len(BOUNDS)
    for name in diffusion_listing:
        assert any(fragment in name for fragment in BOUNDS), f"{name}: a kernel of hns_diffusion.hip without a bound here"


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_diffusion_kernel_resources(diffusion_listing, fragment):
    kernel, vgpr_bound, lds = BOUNDS[fragment]
    found = [m for name, m in diffusion_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == lds, f"{kernel}: {m['group_segment_fixed_size']} bytes of LDS, stated {lds}"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
