"""Registers, LDS and spills of the kernels of hns_point_motion.hip (k_move_points<false | true>), read from the device listing as tests/test_points_collide_resources.py
reads them for hns_points_collide.hip.

Bounds: nothing spills, nothing uses scratch, no kernel uses LDS, and no kernel's VGPR count may pass the allocation granule (8 registers) the first accepted build sits
in. That build has: k_move_points<false> (mode FREE: U only) 56 VGPRs (bound 56), k_move_points<true> (the collider's modes) 72 (bound 72). k_trace_points_collide<1>, which
runs the same samplers, has 61: the eleven more hold the point's velocity, its age and the host's constants of the drag and the reflection across the sampler body. 72 is
seven waves per SIMD, below the 80 from which on it would be six. The six neighbour samples of a bounce run through ONE rolled sampler body, as the push's do."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound)
BOUNDS = {
    "13k_move_pointsILb0E": ("k_move_points<false>", 56),
    "13k_move_pointsILb1E": ("k_move_points<true>", 72),
}


@pytest.fixture(scope="module")
def motion_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_point_motion.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_bounded(motion_listing):
    assert len(motion_listing) == len(BOUNDS)
    for name in motion_listing:
        assert any(fragment in name for fragment in BOUNDS), f"{name}: a kernel of hns_point_motion.hip without a bound here"


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_motion_kernel_resources(motion_listing, fragment):
    kernel, vgpr_bound = BOUNDS[fragment]
    found = [m for name, m in motion_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == 0, f"{kernel} uses LDS"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
