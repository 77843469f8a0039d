"""Registers, LDS and spills of the kernels of hns_seed.hip (k_seed_keys, k_seed_compact, k_seed_masks), read from the kernel metadata of the device listing as
tests/test_splat_resources.py reads them for hns_splat.hip: every kernel of the file is listed, nothing spills, nothing uses scratch, nothing uses LDS. The register counts
of the first accepted build are recorded in DESIGN.md (section 4); they are not gated here beyond that."""
import os
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, kernel_metadata

# mangled-name fragment: kernel
KERNELS = {
    "11k_seed_keys": "k_seed_keys",
    "14k_seed_compact": "k_seed_compact",
    "12k_seed_masks": "k_seed_masks",
}


@pytest.fixture(scope="module")
def seed_listing():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be produced here")
    target = "../lib/obj/hns_seed.hip.s"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(CSRC, target)) as f:
        return kernel_metadata(f.read())


def test_every_kernel_of_the_file_is_checked(seed_listing):
    assert len(seed_listing) == len(KERNELS)
    for name in seed_listing:
        assert any(fragment in name for fragment in KERNELS), f"{name}: a kernel of hns_seed.hip that is not checked here"


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_seed_kernel_resources(seed_listing, fragment):
    kernel = KERNELS[fragment]
    found = [m for name, m in seed_listing.items() if fragment in name]
    assert len(found) == 1, f"{kernel}: {len(found)} kernels match {fragment}"
    m = found[0]
    print(f"{kernel}: vgpr {m['vgpr_count']}, sgpr {m['sgpr_count']}, lds {m['group_segment_fixed_size']}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, f"{kernel} spills"
    assert m["private_segment_fixed_size"] == 0, f"{kernel} uses scratch"
    assert m["group_segment_fixed_size"] == 0, f"{kernel} uses LDS"
