"""hns_dev_sample_points, hns_dev_trace_points, hns_sim_sample_points and hns_sim_trace_points without a GPU: the four symbols are exported by libhns.so,
declared in include/hns.h and bound in hnanosolver_amd/_lib.py, their Python mirrors exist, and without a device they fail loudly (HNS_ERR_NO_DEVICE), as
every compute entry point does. What they compute is held bit for bit to the oracle and the reference's samplers on the MI355X (tests/test_points_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hnanosolver_amd import _lib, api, device, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_dev_sample_points", "hns_dev_trace_points", "hns_sim_sample_points", "hns_sim_trace_points")


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_declared_and_bound(name):
    lib = _lib.load_library()
    assert getattr(lib, name) is not None  # AttributeError: libhns.so does not export it
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        header = f.read()
    assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), f"{name} is not declared in include/hns.h"
    assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    # one ctypes argument per parameter of the declaration
    decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M | re.S).group(1)
    assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1


def test_header_says_the_calls_are_not_mirrored_in_the_partitioned_sim():
    with open(os.path.join(ROOT, "include", "hns.h")) as f:
        header = f.read()
    for name in ("hns_dev_trace_points", "hns_sim_trace_points"):
        comment = header[: header.index("int " + name)].rsplit("/*", 1)[1]
        assert "mirrored in hns_dist_*" in comment, name


def test_python_mirrors_exist():
    assert callable(device.sample_points) and callable(device.trace_points)
    assert callable(device.Sim.sample) and callable(device.Sim.trace)


def test_all_four_fail_loudly_without_a_device():
    lib = _lib.load_library()
    if lib.hns_device_count() > 0:
        pytest.skip("a HIP device is present; this test is for the CPU-only container")
    o = fields.dense_leaves(16)
    h = api.create_grid_from_leaves(o, 1.0 / 16, _lib.HNS_GRID_HOST_ONLY)
    n, npts = len(o) * 512, 5
    vel, rho = np.ones((n, 3), np.float32), np.ones(n, np.float32)
    xyz = np.full((npts, 3), 3.25, np.float32)
    out_f, out_v, status = np.full(npts, 7.0, np.float32), np.full((npts, 3), 7.0, np.float32), np.full(npts, 9, np.uint8)
    ins, outs = (C.c_void_p * 2)(rho.ctypes.data, vel.ctypes.data), (C.c_void_p * 2)(out_f.ctypes.data, out_v.ctypes.data)
    ncomp = (C.c_int * 2)(1, 3)
    assert lib.hns_dev_sample_points(h.ptr, ins, ncomp, 2, xyz.ctypes.data, npts, outs, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_dev_sample_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    assert lib.hns_dev_trace_points(h.ptr, vel.ctypes.data, xyz.ctypes.data, npts, 0.04, 16.0, 2, 1, status.ctypes.data, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_dev_trace_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    # no sim exists without a device: its creation is refused, and the two sim calls say the same of the null they are then handed
    with pytest.raises(_lib.HNSError) as e:
        device.Sim(h, ["density"])
    assert e.value.code == _lib.HNS_ERR_NO_DEVICE
    names = (C.c_char_p * 1)(b"density")
    assert lib.hns_sim_sample_points(None, names, 1, 1, xyz.ctypes.data, npts, outs, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_sim_sample_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    assert lib.hns_sim_trace_points(None, xyz.ctypes.data, npts, 0.04, 1.0 / 16, 4, 2, status.ctypes.data, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_sim_trace_points" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
    assert (out_f == 7.0).all() and (out_v == 7.0).all() and (status == 9).all() and (xyz == np.float32(3.25)).all()
