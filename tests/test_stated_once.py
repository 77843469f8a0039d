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


# The halo exchange (hns_dist_substep.hip): one pack / unpack kernel, one walk over a message's fields (`before +=`), one place that derives the transport
# (hnsd::transport in hns_dist.hpp, so the spelled-out test of its members is gone from this file). (text, how often it may occur in the file)
DIST_SUBSTEP = os.path.join(CSRC, "hns_dist_substep.hip")
DIST_COUNTS = [("k_halo_copy_all", 0), ("before +=", 1), ("!d->comm && !d->loopback && !d->ipc", 0)]


@pytest.mark.parametrize("text,count", DIST_COUNTS)
def test_halo_exchange_stated_once(text, count):
    with open(DIST_SUBSTEP, errors="replace") as f:
        found = [i for i, line in enumerate(f, 1) for _ in range(line.count(text))]
    assert len(found) == count, f"`{text}` occurs {len(found)} times in hns_dist_substep.hip, lines {found}"


def test_halo_copy_kernel_is_launched_by_one_function():
    """every `hipLaunchKernelGGL((k_halo_copy<` lies in the body of one function: between the same two lines that start at column 0 (a definition's
    head and its closing brace)"""
    with open(DIST_SUBSTEP, errors="replace") as f:
        lines = f.read().split("\n")
    launches = [i for i, line in enumerate(lines) if "hipLaunchKernelGGL((k_halo_copy<" in line]
    assert launches, "the pack / unpack kernel is launched nowhere"
    heads = {max(j for j in range(i) if lines[j] and not lines[j][0].isspace() and not lines[j].startswith(("}", "//"))) for i in launches}
    assert len(heads) == 1, [lines[h] for h in sorted(heads)]
    head = heads.pop()
    end = min(j for j in range(head + 1, len(lines)) if lines[j].startswith("}"))
    assert max(launches) < end, (lines[head], launches, end)
