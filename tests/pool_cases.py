"""TEST HELPER of tests/test_pool_contents_gpu.py: option arena_fill (include/hns.h) makes the pool of device memory hand out every block filled with one byte,
so that a result which depends on what pooled memory held differs from fill to fill. The fills, the switch, and the runner that takes a scenario through them."""
import contextlib

import numpy as np
import pytest

import hnanosolver_amd as H

# 0x00: what a fresh process mostly gets from the driver. 0xFF: a NaN as a float, -1 as an int (the library's own "absent" marker), every bit set as a mask.
# 0x7F: 0x7F7F7F7F = 3.39e38, finite -- the BFECC limiter's v_min / v_max and leaf_record let a NaN lose, so a NaN fill alone can be swallowed.
FILLS = (0x00, 0xFF, 0x7F)


@contextlib.contextmanager
def arena_fill(byte):
    """every block the pool hands out inside the block holds `byte`; the switch is off again afterwards, also after an exception"""
    H.set_option("arena_fill", str(int(byte)))
    try:
        yield
    finally:
        H.set_option("arena_fill", None)


def as_bytes(v) -> bytes:
    """a documented output as bytes: arrays as they lie in memory (so that NaN payloads and signed zeros count), counts and reports by their text"""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    return repr(v).encode()


def run_under_fills(scenario, fills=FILLS):
    """scenario() once per fill, in the order of `fills` (a failure under one fill ends the run before the next) -> {fill: {name: bytes}} of the outputs it
    returns. The scenario itself asserts what has an independent reference."""
    out = {}
    for fill in fills:
        with arena_fill(fill):
            out[fill] = {k: as_bytes(v) for k, v in scenario().items()}
    return out


def assert_fills_agree(results):
    """every named output is the same bytes under every fill"""
    (base, first), *rest = results.items()
    assert first, "the scenario returned no outputs"
    for fill, named in rest:
        assert named.keys() == first.keys(), (fill, sorted(named.keys() ^ first.keys()))
        for k, want in first.items():
            got = named[k]
            if got == want:
                continue
            n = min(len(got), len(want))
            at = next((i for i in range(n) if got[i] != want[i]), n)
            raise AssertionError(f"{k}: fill 0x{fill:02X} and fill 0x{base:02X} give different bytes ({len(got)} / {len(want)}), first at byte {at} "
                                 f"(32-bit word {at // 4}, leaf {at // 2048} of a float field)")


def under_every_fill(scenario, fills=FILLS):
    results = run_under_fills(scenario, fills)
    assert_fills_agree(results)
    return results


def check_arena_fill_option():
    """set, get, default, a refused value (host code: needs no device)"""
    assert H.get_option("arena_fill") == "off"
    try:
        for byte in FILLS + (1, 255):
            H.set_option("arena_fill", str(byte))
            assert H.get_option("arena_fill") == str(byte)
        H.set_option("arena_fill", "off")
        assert H.get_option("arena_fill") == "off"
        H.set_option("arena_fill", "127")
        for bad in ("256", "-1", "0x7F", "on", ""):
            with pytest.raises(H.HNSError):
                H.set_option("arena_fill", bad)
            assert H.get_option("arena_fill") == "127", bad  # a refused value changes nothing
        H.set_option("arena_fill", None)
        assert H.get_option("arena_fill") == "off"
    finally:
        H.set_option("arena_fill", None)
