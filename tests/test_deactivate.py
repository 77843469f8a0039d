"""CPU checks of the end-of-frame deactivation's host mirror (hns_deactivate_leaf_masks) against a numpy brute force -- planted signed zeros,
NaN, infinities and values at the tolerance and one float above it -- and its refusals through the Python binding."""
import ctypes as C

import numpy as np
import pytest

from frame_cases import pack, unpack
from hnanosolver_amd import _lib, leafio


def brute_force(masks, n, fields, velocity):
    """voxel by voxel: active stays active iff some listed component has NOT |x| <= tol"""
    active = np.ones((n, 512), dtype=bool) if masks is None else unpack(masks)
    loud = np.zeros((n, 512), dtype=bool)
    with np.errstate(invalid="ignore"):
        for v, t in fields.values():
            loud |= ~(np.abs(np.asarray(v, dtype=np.float32).reshape(n, 512)) <= np.float32(t))
        if velocity is not None:
            v, t = velocity
            loud |= ~(np.abs(np.asarray(v, dtype=np.float32).reshape(n, 512, 3)) <= np.float32(t)).all(axis=2)
    out = active & loud
    return pack(out), (int(out.sum()), int(out.any(axis=1).sum()))


def planted(rng, shape, tol):
    """standard normal values scaled down so that many fall within tol, with +-0, NaN, +-inf and +-tol / the next float above planted"""
    v = (rng.standard_normal(shape) * (2.0 * tol if np.isfinite(tol) and tol > 0 else 1.0)).astype(np.float32)
    flat = v.reshape(-1)
    t = np.float32(tol)
    above = np.nextafter(t, np.float32(np.inf))
    specials = [np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), t, -t, above, -above]
    for sv in specials:
        flat[rng.random(flat.size) < 0.02] = sv
    quiet = rng.random(flat.size) < 0.3  # long quiet stretches, so that whole words and leaves clear
    flat[quiet] = np.where(rng.random(quiet.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    return v


def random_masks(rng, n):
    bits = rng.random((n, 512)) < rng.choice([0.0, 0.02, 0.5, 1.0], size=(n, 1))
    bits[:, 64:128] = False  # a whole word empty on every leaf (the kernel skips it)
    return pack(bits)


def state(seed, n, names, tols, vel_tol):
    rng = np.random.default_rng(seed)
    fields = {k: (planted(rng, (n * 512,), tols[k]), tols[k]) for k in names}
    velocity = None if vel_tol is None else (planted(rng, (n * 512, 3), vel_tol), vel_tol)
    if n > 3:  # leaves whose every listed value is quiet: they must lose every bit
        for v, _ in list(fields.values()) + ([velocity] if velocity else []):
            v.reshape(n, -1)[1:3] = 0.0
    return rng, fields, velocity


TOLS = {"zero": 0.0, "small": 1e-3, "one": 1.0, "inf": float("inf")}


@pytest.mark.parametrize("masked", [False, True], ids=["nullmasks", "masks"])
@pytest.mark.parametrize("tol", list(TOLS))
@pytest.mark.parametrize("kind", ["velocity", "floats", "mixed"])
def test_host_mirror_against_brute_force(kind, tol, masked):
    n = 17
    t = TOLS[tol]
    names = [] if kind == "velocity" else ["density", "temperature"]
    tols = {k: (t if i == 0 else TOLS["small"] if t != TOLS["small"] else 0.5) for i, k in enumerate(names)}
    rng, fields, velocity = state(len(kind) * 7 + len(tol) + masked, n, names, tols, None if kind == "floats" else t)
    masks = random_masks(rng, n) if masked else None
    before = None if masks is None else masks.copy()
    got, counts = leafio.deactivate_masks(masks, fields, velocity)
    want, want_counts = brute_force(masks, n, fields, velocity)
    assert np.array_equal(got, want)
    assert counts == want_counts
    if masks is not None:
        assert np.array_equal(masks, before), "the input masks are not written"
        assert not (unpack(got) & ~unpack(masks)).any(), "bits are only ever cleared"
    if t != float("inf") or kind != "velocity":
        assert (got[1:3] == 0).all(), "leaves with every listed value quiet lose every bit"


def test_special_values_one_by_one():
    """one leaf, density only, every voxel a chosen value: exactly the values that are not within tolerance stay active"""
    t = np.float32(0.25)
    vals = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, t, -t, np.nextafter(t, np.float32(1)), -np.nextafter(t, np.float32(1)), 0.1, 1e-30],
                    dtype=np.float32)
    keep = np.array([0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0], dtype=bool)
    v = np.zeros(512, dtype=np.float32)
    v[: len(vals)] = vals
    got, counts = leafio.deactivate_masks(None, {"density": (v, t)})
    bits = unpack(got)[0]
    assert np.array_equal(bits[: len(vals)], keep) and not bits[len(vals):].any()
    assert counts == (int(keep.sum()), 1)
    # +inf tolerance: everything but NaN is within
    got, counts = leafio.deactivate_masks(None, {"density": (v, float("inf"))})
    assert np.array_equal(unpack(got)[0, : len(vals)], np.isnan(vals)) and counts == (2, 1)
    # the velocity: a voxel is quiet only if all three components are
    vel = np.zeros((512, 3), dtype=np.float32)
    vel[0] = [-0.0, 0.0, -0.0]
    vel[1] = [0.0, 0.0, 1e-38]
    vel[2] = [np.nan, 0.0, 0.0]
    vel[3, 2] = -1e-45
    got, counts = leafio.deactivate_masks(None, {}, (vel, 0.0))
    assert np.array_equal(np.flatnonzero(unpack(got)[0]), [1, 2, 3]) and counts == (3, 1)


def test_all_quiet_clears_everything_and_counts_zero():
    n = 5
    got, counts = leafio.deactivate_masks(None, {"density": (np.zeros(n * 512, np.float32), 0.0)}, (np.full((n * 512, 3), -0.0, np.float32), 0.0))
    assert (got == 0).all() and counts == (0, 0)


def test_in_place_and_word_layout():
    """masks_out may be masks_in; mask byte x*8+y bit z is voxel x*64+y*8+z"""
    n = 3
    rng = np.random.default_rng(5)
    m = random_masks(rng, n)
    v = rng.standard_normal(n * 512).astype(np.float32)
    v[::3] = 0.0
    want, wc = brute_force(m, n, {"density": (v, 0.0)}, None)
    lib = _lib.load_library()
    arr, nf = leafio.activity_fields({"density": 0.0})
    ptrs = (C.c_void_p * 1)(v.ctypes.data)
    counts = (C.c_uint64 * 2)()
    assert lib.hns_deactivate_leaf_masks(n, m.ctypes.data, arr, ptrs, nf, m.ctypes.data, counts) == _lib.HNS_OK
    assert np.array_equal(m, want) and (counts[0], counts[1]) == wc
    one = np.zeros(512, np.float32)
    one[3 * 64 + 5 * 8 + 6] = 1.0
    got, _ = leafio.deactivate_masks(None, {"density": (one, 0.0)})
    assert got[0, 3 * 8 + 5] == 1 << 6 and got.sum() == 1 << 6


def raw(entries, n=1, masks=None, values=None, counts=True):
    """hns_deactivate_leaf_masks with hand-built entries (name, ncomp, tolerance) -> (code, message, masks_out)"""
    lib = _lib.load_library()
    arr = (_lib.hns_activity_field * max(1, len(entries)))()
    for i, (name, nc, tol) in enumerate(entries):
        arr[i].name, arr[i].ncomp, arr[i].tolerance = None if name is None else name.encode(), nc, tol
    vals = values if values is not None else [np.ones(n * 512 * (3 if nc == 3 else 1), np.float32) for _, nc, _ in entries]
    ptrs = (C.c_void_p * max(1, len(vals)))(*[None if v is None else v.ctypes.data for v in vals])
    out = np.full((n, 64), 0xA5, dtype=np.uint8)
    cnt = (C.c_uint64 * 2)()
    rc = lib.hns_deactivate_leaf_masks(n, None if masks is None else masks.ctypes.data, arr if entries is not None else None, ptrs, len(entries), out.ctypes.data,
                                       cnt if counts else None)
    return rc, lib.hns_last_error().decode(), out


def test_host_mirror_refusals():
    cases = [
        ([], "bad field list"),
        ([("density", 2, 0.0)], "ncomp 2"),
        ([("density", 0, 0.0)], "ncomp 0"),
        ([("collision_sdf", 1, 0.0)], "'collision_sdf' cannot be deactivated"),
        ([(None, 1, 0.0)], "a float field needs a name"),
        ([("density", 1, 0.0), ("fuel", 1, 0.0), ("density", 1, 1.0)], "a second entry for 'density'"),
        ([("vel", 3, 0.0), ("v2", 3, 0.0)], "a second velocity entry"),
        ([(None, 3, 0.0), (None, 3, 0.0)], "a second velocity entry"),
        ([("density", 1, -1.0)], "tolerance -1"),
        ([("density", 1, -0.0), ("fuel", 1, float("nan"))], "tolerance nan"),
        ([("vel", 3, float("-inf"))], "tolerance -inf"),
    ]
    for entries, msg in cases:
        rc, text, out = raw(entries)
        assert rc == _lib.HNS_ERR_INVALID_ARGUMENT, (entries, rc, text)
        assert text.startswith("hns_deactivate_leaf_masks:") and msg in text, text
        assert (out == 0xA5).all(), "a refusal writes no mask"
    rc, text, out = raw([("density", 1, 0.0)], values=[None])
    assert rc == _lib.HNS_ERR_INVALID_ARGUMENT and "values NULL" in text and (out == 0xA5).all()
    lib = _lib.load_library()
    out = np.zeros(64, np.uint8)
    assert lib.hns_deactivate_leaf_masks(1, None, None, None, 1, out.ctypes.data, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert "NULL list" in lib.hns_last_error().decode()
    # -0.0 and +inf are legal tolerances; no leaves is legal
    assert raw([("density", 1, -0.0), (None, 3, float("inf"))])[0] == _lib.HNS_OK
    assert raw([("density", 1, 0.0)], n=0)[0] == _lib.HNS_OK
    # through leafio: the same refusals as exceptions
    with pytest.raises(_lib.HNSError, match="bad field list"):
        leafio.deactivate_masks(np.zeros((1, 64), np.uint8), {})
    with pytest.raises(_lib.HNSError, match="tolerance nan"):
        leafio.deactivate_masks(None, {"density": (np.zeros(512, np.float32), float("nan"))})
    with pytest.raises(ValueError, match="need 2 x 512 x 3 floats"):
        leafio.deactivate_masks(np.zeros((2, 64), np.uint8), {}, (np.zeros((512, 3), np.float32), 0.0))


def test_sim_deactivate_binding_refuses_a_null_sim():
    lib = _lib.load_library()
    arr, n = leafio.activity_fields({"density": 0.0}, 0.0)
    assert lib.hns_sim_deactivate(None, arr, n, None, None) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert "hns_sim_deactivate: null sim" in lib.hns_last_error().decode()
    for name in ("hns_sim_deactivate", "hns_deactivate_leaf_masks"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert [f[0] for f in _lib.hns_activity_field._fields_] == ["name", "ncomp", "tolerance"]
