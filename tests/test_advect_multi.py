"""hns_dev_advect_scalar_multi and hns_sim_advect without a GPU: the two symbols are exported by libhns.so, declared in include/hns.h and bound in
hnanosolver_amd/_lib.py, and without a device they fail loudly (HNS_ERR_NO_DEVICE), as every compute entry point does. What they compute is held bit for
bit to the single-field kernel, the oracle and the reference on the MI355X (tests/test_advect_multi_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hnanosolver_amd import _lib, api, device, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hns_dev_advect_scalar_multi", "hns_sim_advect")


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


def test_python_mirrors_exist():
    assert callable(device.advect_scalar_multi) and callable(device.Sim.advect)


def test_both_fail_loudly_without_a_device():
    lib = _lib.load_library()
    if lib.hns_device_count() > 0:
        pytest.skip("a HIP device is present; this test is for the CPU-only container")
    o = fields.dense_leaves(16)
    h = api.create_grid_from_leaves(o, 1.0 / 16, _lib.HNS_GRID_HOST_ONLY)
    n = len(o) * 512
    vel, src, dst = np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.full(n, 7.0, np.float32)
    ins, outs = (C.c_void_p * 1)(src.ctypes.data), (C.c_void_p * 1)(dst.ctypes.data)
    assert lib.hns_dev_advect_scalar_multi(h.ptr, vel.ctypes.data, ins, outs, 1, None, 0, 0.04, 16.0, None) == _lib.HNS_ERR_NO_DEVICE
    assert "no CPU fallback" in lib.hns_last_error().decode()
    assert (dst == 7.0).all()
    # no sim exists without a device: its creation is refused, and hns_sim_advect says the same of the null it is then handed
    with pytest.raises(_lib.HNSError) as e:
        device.Sim(h, ["density"])
    assert e.value.code == _lib.HNS_ERR_NO_DEVICE
    names = (C.c_char_p * 1)(b"density")
    assert lib.hns_sim_advect(None, names, 1, 1, 0.04, 1.0 / 16, None) == _lib.HNS_ERR_NO_DEVICE
    assert "hns_sim_advect" in lib.hns_last_error().decode() and "no CPU fallback" in lib.hns_last_error().decode()
