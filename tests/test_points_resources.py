"""Registers, LDS and spills of the kernels of hns_points.hip (k_sample_points, k_trace_points<1 | 2 | 4>), read from the device listing as
tests/test_kernel_resources.py reads them for the advection kernels.

Bounds: nothing spills, nothing uses scratch, no kernel uses LDS, and no kernel's VGPR count may pass the allocation granule (8 registers) the first accepted build sits
in. That build has: k_sample_points 74 VGPRs (bound 80), k_trace_points<1> 47 (bound 48), <2> 51 (56), <4> 67 (72). The kernels wait on dependent gathers, so the waves per
SIMD those granules allow (512 / granule, at most 8) are what hides their latency."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: (kernel, VGPR bound)
BOUNDS = {
    "15k_sample_points": ("k_sample_points", 80),
    "14k_trace_pointsILi1E": ("k_trace_points<1>", 48),
    "14k_trace_pointsILi2E": ("k_trace_points<2>", 56),
    "14k_trace_pointsILi4E": ("k_trace_points<4>", 72),
}


@pytest.fixture(scope="module")
def points_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_points.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_bounded(points_listing):
    for name in points_listing:
        assert any(fragment in name for fragment in BOUNDS), f"{name}: a kernel of hns_points.hip without a bound here"


@pytest.mark.parametrize("fragment", sorted(BOUNDS))
def test_point_kernel_resources(points_listing, fragment):
    kernel, vgpr_bound = BOUNDS[fragment]
    found = [m for name, m in points_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']} (<= {vgpr_bound}), sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == 0, f"{kernel} uses LDS"
    assert m["vgpr_count"] <= vgpr_bound, f"{kernel}: {m['vgpr_count']} VGPRs, bound {vgpr_bound}"
