"""Each reference expression of the projection is written out once in hnanosolver_amd/csrc (hns_device.hpp) and every kernel that needs it calls that one
statement: the Gauss-Seidel value's 1/6 (Kernel.cu:609), combustion's flame term (Kernel.cu:957), buoyancy's force (Kernel.cu:844) and the wave-level LDS
fence. Copies used to be kept in step by the bit-parity tests alone."""
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hnanosolver_amd", "csrc")

ONCE = ["0.166666667f", "burn * 10.0f", "fmaxf(0.0f, tempDiff * strength)", "wave_barrier"]


@pytest.mark.parametrize("text", ONCE)
def test_stated_exactly_once(text):
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path):
            with open(path, errors="replace") as f:
                found += [f"{os.path.basename(path)}:{i}" for i, line in enumerate(f, 1) for _ in range(line.count(text))]
    assert len(found) == 1, f"`{text}` occurs {len(found)} times in hnanosolver_amd/csrc: {found}"
    assert found[0].startswith("hns_device.hpp:"), found
