"""Registers, LDS and spills of the kernels of hns_shaping.hip (k_shape<false | true>), read from the device listing as tests/test_point_motion_resources.py reads them
for hns_point_motion.hip.

Bounds: nothing spills, nothing uses scratch, and no kernel's VGPR count may pass the allocation granule (8 registers) the first accepted build sits in. That build has:
k_shape<true> (turbulence, with or without decays) 71 VGPRs (bound 72: seven waves per SIMD by registers, so three 512-thread workgroups per CU) -- the file is built
without the SLP vectoriser, which pairs the arithmetic into packed f32 at 146 registers and one workgroup per CU --, k_shape<false> (decays alone) 5 (bound 8). LDS:
k_shape<true> holds the gradient table as 16 x 4 floats, 256 bytes, and nothing else; k_shape<false> uses none."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound, LDS bytes)
BOUNDS = {
    "7k_shapeILb0E": ("k_shape<false>", 8, 0),
    "7k_shapeILb1E": ("k_shape<true>", 72, 16 * 4 * 4),
}


@pytest.fixture(scope="module")
def shaping_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_shaping.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_bounded(shaping_listing):
    assert len(shaping_listing) == len(BOUNDS)
    for name in shaping_listing:
        assert any(fragment in name for fragment in BOUNDS), f"{name}: a kernel of hns_shaping.hip without a bound here"


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_shaping_kernel_resources(shaping_listing, fragment):
    kernel, vgpr_bound, lds = BOUNDS[fragment]
    found = [m for name, m in shaping_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == lds, f"{kernel}: {m['group_segment_fixed_size']} bytes of LDS, stated {lds}"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
