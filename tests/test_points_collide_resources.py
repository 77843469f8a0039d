"""Registers, LDS and spills of the kernels of hns_points_collide.hip (k_trace_points_collide<1 | 2 | 4>), read from the device listing as
tests/test_points_resources.py reads them for hns_points.hip.

Bounds: nothing spills, nothing uses scratch, no kernel uses LDS, and no kernel's VGPR count may pass the allocation granule (8 registers) the first accepted build sits
in. That build has: k_trace_points_collide<1> 61 VGPRs (bound 64), <2> 62 (64), <4> 69 (72): order 4 runs at the seven waves per SIMD of k_trace_points<4> (67 registers),
orders 1 and 2 at eight, in the granule above their plain kernels' (47, 51). The six neighbour samples of a push run through ONE rolled sampler body: unrolled they are issued
together and the same build needs 149 to 152 registers (three waves per SIMD), whatever the share of points that ever push."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound)
BOUNDS = {
    "22k_trace_points_collideILi1E": ("k_trace_points_collide<1>", 64),
    "22k_trace_points_collideILi2E": ("k_trace_points_collide<2>", 64),
    "22k_trace_points_collideILi4E": ("k_trace_points_collide<4>", 72),
}


@pytest.fixture(scope="module")
def collide_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_points_collide.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_bounded(collide_listing):
    assert len(collide_listing) == len(BOUNDS)
    for name in collide_listing:
        assert any(fragment in name for fragment in BOUNDS), f"{name}: a kernel of hns_points_collide.hip without a bound here"


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_collide_kernel_resources(collide_listing, fragment):
    kernel, vgpr_bound = BOUNDS[fragment]
    found = [m for name, m in collide_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == 0, f"{kernel} uses LDS"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
