"""The operand contract of include/hns.h ("Device operands"), held on the GPU: a device pointer needs the alignment of its element type and no more, results do not
depend on it, an output may overlap an input only where a function says so, and where a function says "must not alias" any overlap is refused.

Every case of tests/layout_cases.py runs with ALL its operands carved from one guard-banded slab a few bytes behind a multiple of 256 (layouts "plus4" and "mixed") and
must give, byte for byte, what the same call gives on separately allocated tensors and what the oracle or host mirror says; the guards must be intact and the inputs
unchanged. Then the two places where the library picks a kernel path by pointer bits and only one had a test (the float finish of the splat), the harness itself (a
stand-in call that stores through a pointer rounded down to 16 bytes must be reported), the calls that may run in place, and the refusals. No tolerance anywhere."""
import numpy as np
import pytest

import hnanosolver_amd as H
import layout_cases as lc
import stream_cases as sc
from stream_cases import N_POINTS, NS, Call, F

pytestmark = pytest.mark.gpu

OPTIONS = ("rbgs", "sor_block_lb", "stencil")
_CTX = {}


def ctx(name):
    if name not in _CTX:
        _CTX[name] = sc.Ctx(name)
    return _CTX[name]


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(autouse=True)
def default_options():
    yield
    for k in OPTIONS:
        H.set_option(k, None)


def _D():
    from hnanosolver_amd import device

    return device


CASES = [(n, v, g, layout) for n, v, g in lc.variants() for layout in lc.LAYOUTS]


@pytest.mark.parametrize("name,variant,grid,layout", CASES, ids=[f"{n}-{v}-{g}-{layout}" for n, v, g, layout in CASES])
def test_call_gives_the_same_bytes_at_element_alignment(name, variant, grid, layout, torch):
    lc.check_layout(torch, ctx(grid), name, variant, layout)


# ---------------------------------------------------------------------------------------------------------------
# the splat's float finish on a field that is not 16-byte aligned
# ---------------------------------------------------------------------------------------------------------------


def splat_three_fields(x, through_order):
    def run(t):
        D = _D()
        fields, vals = [t.density, t.fuel, t.vel], [t.vals, t.vals_b, t.vals3]
        if through_order:
            with lc._order(x, t) as o:
                o.splat(fields, t.xyz, vals, status=t.status, rejected=t.rejected)
        else:
            D.splat_points(x.grid, fields, t.xyz, vals, status=t.status, rejected=t.rejected)

    def expect(h):
        from hnanosolver_amd import api

        fields, status = [np.array(h.density), np.array(h.fuel), np.array(h.vel)], np.zeros(N_POINTS, np.uint8)
        rejected = api.splat_points_host(x.grid, fields, h.xyz, [h.vals, h.vals_b, h.vals3], status=status)
        return {"density": fields[0], "fuel": fields[1], "vel": fields[2], "status": status, "rejected": np.array([rejected], dtype=np.int64)}

    vals_b = np.random.default_rng(51).standard_normal(N_POINTS).astype(F)
    ins = {"density": x.f["density"], "fuel": x.f["fuel"], "vel": x.f["vel"], "xyz": lc._splat_points(x), "vals": x.values, "vals_b": vals_b, "vals3": x.values3,
           "rejected": np.zeros(1, np.int64)}
    return Call(ins, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("density", "fuel", "vel", "rejected"))


@pytest.mark.parametrize("through_order", [False, True], ids=["hns_dev_splat_points", "hns_point_order_splat"])
def test_splat_finishes_a_float_field_that_is_not_16_byte_aligned(through_order, torch):
    """two float fields in one call, one 16-byte aligned (the float4 finish) and one 4 bytes behind (the stride-1 scalar finish), and a Vec3f field, held to the mirror"""
    x = ctx("scattered")
    call = splat_three_fields(x, through_order)
    got, slab = lc.run_skewed(torch, call, {"fuel": 4}, "splat with fuel at +4")
    assert slab.views.density.data_ptr() % 16 == 0 and slab.views.fuel.data_ptr() % 16 == 4 and slab.views.vel.data_ptr() % 16 == 0
    want = call.expect(NS(call.inputs))
    assert not sc.same_words(want["fuel"], call.inputs["fuel"]) and int(want["status"].max()) == 8  # (the points do change the field)
    for k, v in want.items():
        assert sc.same_words(got[k], v), f"output {k} differs from the host mirror"


# ---------------------------------------------------------------------------------------------------------------
# the harness bites
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_harness_reports_a_rounded_down_store(layout, torch):
    """a torch-only stand-in for a kernel that takes `out & ~15` for its first 16-byte piece: the right bytes, 4 .. 12 bytes too early"""
    x = ctx("scattered")
    call = sc.k_divergence(x)

    def stand_in(t):
        ahead = t.out_ptr % 16
        assert ahead in (4, 8, 12)
        low = torch.empty(0, dtype=torch.uint8, device="cuda").set_(t.div.untyped_storage(), t.div.storage_offset() * 4 - ahead, (x.N * 4,))
        low.copy_(torch.from_numpy(np.array(x.div).view(np.uint8)))

    slab = lc.carve(torch, call, layout, "cuda")
    t = NS(slab.views, out_ptr=slab.views.div.data_ptr())
    slab.check("fresh")
    stand_in(t)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"leading guard of div, (4|8|12) bytes before its start"):
        slab.check("stand-in")


# ---------------------------------------------------------------------------------------------------------------
# permitted aliasing: "out3 may alias vel3"
# ---------------------------------------------------------------------------------------------------------------


def gradient_in_place(coll, options):
    def build(x):
        ins = {"vel": x.f["vel"], "p": x.p, **({"sdf": x.sdf} if coll else {})}
        return Call(ins, {}, lambda t: _D().subtract_pressure_gradient(x.grid, t.vel, t.p, t.vel, x.inv_dx, t.sdf, coll),
                    lambda h: {"vel": x.oracle.subtract_pressure_gradient(h.vel, h.p, x.inv_dx, h.sdf, coll)}, inplace=("vel",), options=options)
    return build


def buoyancy_in_place(x):
    return Call({"vel": x.f["vel"], "temperature": x.f["temperature"]}, {}, lambda t: _D().temperature_buoyancy(t.vel, t.temperature, t.vel, x.dt, 23.0, 1.0),
                lambda h: {"vel": x.oracle.temperature_buoyancy(h.vel, h.temperature, x.dt, 23.0, 1.0)}, inplace=("vel",))


# variant -> (the in-place builder, the out-of-place builder of stream_cases, the kernel the form is)
IN_PLACE = {
    "gradient_plain": (gradient_in_place(False, {}), sc.k_gradient(False), "k_subtract_gradient_s"),
    "gradient_collision": (gradient_in_place(True, {}), sc.k_gradient(True), "k_subtract_gradient<true>"),
    "gradient_stencil_block": (gradient_in_place(False, {"stencil": "block"}), sc.k_gradient(False), "k_subtract_gradient<false>"),
    "buoyancy": (buoyancy_in_place, sc.k_buoyancy, "k_temperature_buoyancy"),
}
_OUT_OF_PLACE = {}
assert {"hns_dev_subtract_pressure_gradient" if v.startswith("gradient") else "hns_dev_temperature_buoyancy" for v in IN_PLACE} == set(lc.MAY_ALIAS)


@pytest.mark.parametrize("layout", ["aligned", "mixed"])
@pytest.mark.parametrize("grid", ["scattered", "plume"])
@pytest.mark.parametrize("variant", sorted(IN_PLACE))
def test_call_in_place_where_the_header_permits_it(variant, grid, layout, torch):
    x = ctx(grid)
    build, out_of_place, _ = IN_PLACE[variant]
    call = build(x)
    try:
        for k, v in call.options.items():
            H.set_option(k, v)
        key = (variant, grid)
        if key not in _OUT_OF_PLACE:
            other = out_of_place(x)
            _OUT_OF_PLACE[key] = (lc.run_plain(torch, other)["out"], call.expect(NS(call.inputs))["vel"])
        apart, oracle = _OUT_OF_PLACE[key]
        what = f"{variant} in place on {grid}, {layout}"
        if layout == "aligned":
            got = lc.run_plain(torch, call)
        else:
            got, slab = lc.run_skewed(torch, call, layout, what)
            assert slab.views.vel.data_ptr() % 16 == 12
        assert sc.same_words(apart, oracle), f"{what}: the out-of-place call differs from the oracle"
        assert sc.same_words(got["vel"], apart), f"{what}: differs from the out-of-place call"
    finally:
        for k in call.options:
            H.set_option(k, None)


# ---------------------------------------------------------------------------------------------------------------
# forbidden aliasing: "must not alias" / "not aliasing"
# ---------------------------------------------------------------------------------------------------------------


LEAF = 512  # the partial overlap of every refusal: the output starts one leaf of its own elements into the input


def _refusal_buffers(torch, x, floats_per_voxel):
    """two fields' worth of floats and a leaf, holding a recognisable pattern -> (tensor, its bytes before the call)"""
    buf = torch.arange(2 * x.N * floats_per_voxel + LEAF * floats_per_voxel, dtype=torch.float32, device="cuda")
    return buf, buf.cpu().numpy().copy()


def _refused(rc, *named):
    from hnanosolver_amd import _lib

    msg = _D().lib.hns_last_error().decode()
    assert rc == _lib.HNS_ERR_INVALID_ARGUMENT, (rc, msg)
    assert any(n in msg for n in named), msg


def _vector_pair(call):
    """call(vel3 pointer, out3 pointer) -> return code"""
    def run(torch, x):
        buf, before = _refusal_buffers(torch, x, 3)
        base = buf.data_ptr()
        for out in (base, base + 4 * 3 * LEAF):  # identical, and one leaf in
            _refused(call(x, base, out), "alias", "overlap")
            torch.cuda.synchronize()
            assert sc.same_words(buf, before), "a refused call wrote"
    return run


def _lib_call(name, args):
    return lambda x, a, b: getattr(_D().lib, name)(*args(x, a, b))


def _ahead(torch, x):
    import ctypes as C

    L = _D().lib
    buf, before = _refusal_buffers(torch, x, 3)
    phi, out = torch.zeros(x.N, device="cuda"), torch.full((x.N,), 7.0, device="cuda")
    ins, outs = (C.c_void_p * 1)(phi.data_ptr()), (C.c_void_p * 1)(out.data_ptr())
    base = buf.data_ptr()
    for adv in (base, base + 4 * 3 * LEAF):
        _refused(L.hns_dev_advect_scalars_ahead(x.grid.ptr, base, ins, outs, 1, adv, x.dt, x.inv_dx, None), "adv_out3")
        torch.cuda.synchronize()
        assert sc.same_words(buf, before) and bool((out == 7.0).all()), "a refused call wrote"


def _rbgs(torch, x):
    L = _D().lib
    buf, before = _refusal_buffers(torch, x, 1)
    div = torch.zeros(x.N, device="cuda")
    base = buf.data_ptr()
    for p_b in (base, base + 4 * LEAF):
        _refused(L.hns_dev_rbgs_iterate(x.grid.ptr, div.data_ptr(), base, p_b, x.vs, x.omega, 4, None, None), "p_a")
    other = torch.zeros(x.N, device="cuda")
    for d in (base, base + 4 * LEAF):  # div over p_a, then over p_b
        _refused(L.hns_dev_rbgs_iterate(x.grid.ptr, d, base, other.data_ptr(), x.vs, x.omega, 4, None, None), "div")
        _refused(L.hns_dev_rbgs_iterate(x.grid.ptr, d, other.data_ptr(), base, x.vs, x.omega, 4, None, None), "div")
    torch.cuda.synchronize()
    assert sc.same_words(buf, before) and bool((div == 0).all()) and bool((other == 0).all()), "a refused call wrote"


def _multi(torch, x):
    import ctypes as C

    L = _D().lib
    buf, before = _refusal_buffers(torch, x, 3)  # (long enough to stand for a velocity)
    vel, phi = torch.zeros((x.N, 3), device="cuda"), torch.zeros(x.N, device="cuda")
    base = buf.data_ptr()

    def call(vel3, in0, out0):
        ins, outs = (C.c_void_p * 1)(in0), (C.c_void_p * 1)(out0)
        return L.hns_dev_advect_scalar_multi(x.grid.ptr, vel3, ins, outs, 1, None, 0, x.dt, x.inv_dx, None)

    _refused(call(vel.data_ptr(), base, base + 4 * LEAF), "aliases the input")
    _refused(call(base, phi.data_ptr(), base + 4 * LEAF), "aliases the velocity")
    torch.cuda.synchronize()
    assert sc.same_words(buf, before) and bool((vel == 0).all()) and bool((phi == 0).all()), "a refused call wrote"


REFUSALS = {
    "hns_dev_advect_vector": _vector_pair(_lib_call("hns_dev_advect_vector", lambda x, a, b: (x.grid.ptr, a, b, None, 0, x.dt, x.inv_dx, None))),
    "hns_dev_vorticity_confinement": _vector_pair(_lib_call("hns_dev_vorticity_confinement", lambda x, a, b: (x.grid.ptr, a, b, x.dt, x.inv_dx, 1.0, 1.0, None))),
    "hns_dev_advect_scalars_ahead": _ahead,
    "hns_dev_rbgs_iterate": _rbgs,
}


assert set(REFUSALS) == set(lc.MUST_NOT_ALIAS)  # (tests/test_layout_cases.py holds that table to the sentences of include/hns.h)


@pytest.mark.parametrize("name", sorted(REFUSALS) + ["hns_dev_advect_scalar_multi"])
def test_overlapping_operands_are_refused_where_the_header_forbids_them(name, torch):
    """identical pointers and an output one leaf into its input: HNS_ERR_INVALID_ARGUMENT with the argument named, before anything is launched -- the buffers keep their bytes"""
    x = ctx("scattered")
    (REFUSALS.get(name) or _multi)(torch, x)
