"""Point values into fields through a leaf order on the GPU: hns_point_order_splat / hns_point_order_splat_sim (k_binned_points, k_binned_leaf of hns_splat_binned.hip)
and their Python wrappers device.PointOrder.splat / device.Sim.splat(order=...).

Every comparison is equality of bytes against the host mirrors hns_grid_splat_points / hns_grid_splat_points_spec (splat_cases.mirror, rasterize_cases.mirror), which the
CPU suites hold to the numpy restatements of include/hns.h: fields, status, the rejected count, masks. There is no tolerance: the sums are integers. The point sets and the
conditions they meet (tail and leaf terms into one voxel, leaves fed by neighbours only, crossings): tests/binned_cases.py."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import binned_cases as bc
import order_cases as oc
import rasterize_cases as rc
import seed_cases as sd
import splat_cases as sp
import stream_cases as sc
from frame_cases import LAUNCH_RANGES, download, launch_range, make_sim, random_state
from pool_cases import arena_fill

pytestmark = pytest.mark.gpu

F = np.float32
VS = 1.0 / 24.0
SENTINEL = 0xAB
REJECTED_BEFORE = 5  # d_rejected is added to, not set
LEVELS = ("leaf", "voxel")


class Rig:
    """a device grid over a leaf set; the host mirror runs on the same grid"""

    def __init__(self, origins):
        import torch

        from hnanosolver_amd import api, device

        self.t, self.D = torch, device
        self.grid = api.create_grid_from_leaves(np.ascontiguousarray(origins, dtype=np.int32), VS)

    def dev(self, a):
        return self.t.from_numpy(np.array(a)).cuda()

    def padded(self, a, fill=7.0):
        """a device tensor one row longer than a, filled with `fill` behind a's rows: no call gets a null pointer for n = 0, and the row behind the last is watched"""
        a = np.asarray(a, dtype=F)
        full = self.t.full((len(a) + 1, *a.shape[1:]), fill, dtype=self.t.float32, device="cuda")
        full[: len(a)] = self.dev(a)
        return full

    def ordered(self, fields, xyz, values, q=-32, level="voxel", rows="original", what="", radii=None, **spec):
        """sort, (rows="ranked": gather,) one PointOrder.splat on copies of the fields -> (new fields, status in the ORIGINAL order, rejected). The per-point arrays and the
        row behind the last of each are watched. radii: one radius per point (then spec's `radius` is their bound)"""
        t, n = self.t, len(xyz)
        xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
        host = [xyz, *[np.asarray(v, dtype=F) for v in values]] + ([np.asarray(radii, dtype=F)] if radii is not None else [])
        full = [self.padded(a) for a in host]
        po = self.D.PointOrder(self.grid, max(n, 1))
        po.sort(full[0][:n], level)
        perm = po.perm.cpu().numpy().view(np.uint32).astype(np.int64)
        if rows == "ranked":
            host = [a[perm] for a in host]
            ranked = [t.full(tuple(f.shape), 7.0, dtype=t.float32, device="cuda") for f in full]
            for src, dst in zip(full, ranked):
                po.gather(src, dst)
            full = ranked
        d_fields = [self.dev(f) for f in fields]
        status = t.full((n + 1,), SENTINEL, dtype=t.uint8, device="cuda")
        rejected = t.full((1,), REJECTED_BEFORE, dtype=t.int64, device="cuda")
        if radii is not None:
            spec = dict(spec, max_radius=spec["radius"], radius=full[-1][:n])
        po.splat(d_fields, full[0][:n], [f[:n] for f in full[1 : 1 + len(values)]], q, status[:n], rejected, rows=rows, **spec)
        st = status.cpu().numpy()
        assert st[n] == SENTINEL, f"{what}: status was written behind its last byte"
        for f, a in zip(full, host):
            got = f.cpu().numpy()
            assert sp.same_bytes(got[:n], a) and (got[n:] == 7.0).all(), f"{what}: a per-point array changed"
        po.close()
        back = np.empty(n, dtype=np.uint8)
        back[perm if rows == "ranked" else np.arange(n)] = st[:n]
        return [f.cpu().numpy() for f in d_fields], back, int(rejected.cpu().numpy()[0]) - REJECTED_BEFORE

    def plain(self, fields, xyz, values, q=-32, **spec):
        """hns_dev_splat_points on copies -> new fields"""
        d_fields = [self.dev(f) for f in fields]
        self.D.splat_points(self.grid, d_fields, self.dev(np.asarray(xyz, dtype=F).reshape(-1, 3)), [self.dev(v) for v in values], q, **spec)
        return [f.cpu().numpy() for f in d_fields]


@functools.lru_cache(maxsize=None)
def rig(name):
    return Rig(oc.origins(name) if name == "dense64" else bc.case(name)["o"])


def freeze(fields, xyz, values):
    return tuple(np.asarray(a).tobytes() for a in [*fields, xyz, *values])


_mirrors = {}


def mirror(R, fields, xyz, values, q=-32, radii=None, **spec):
    """the host mirror of one call, computed once per input (the ordered calls of all levels and row layouts share it) -> (fields, status, rejected)"""
    key = (id(R), freeze(fields, xyz, values), q, None if radii is None else np.asarray(radii).tobytes(), tuple(sorted(spec.items())))
    if key not in _mirrors:
        if len(_mirrors) > 8:
            _mirrors.clear()
        host_spec = dict(spec, max_radius=spec["radius"], radius=np.ascontiguousarray(radii, dtype=F)) if radii is not None else spec
        _mirrors[key] = rc.mirror(R.grid, fields, np.asarray(xyz, dtype=F).reshape(-1, 3), values, q, **host_spec)[:3]
    return _mirrors[key]


def assert_equal_the_mirror(R, fields, xyz, values, what, q=-32, level="voxel", rows="original", radii=None, changes=True, **spec):
    got, status, rej = R.ordered(fields, xyz, values, q, level, rows, what, radii, **spec)
    want, want_status, want_rej = mirror(R, fields, xyz, values, q, radii, **spec)
    for i in range(len(fields)):
        d = np.flatnonzero(got[i].reshape(-1).view(np.uint32) != want[i].reshape(-1).view(np.uint32))
        assert len(d) == 0, f"{what}: field {i}: {len(d)} words differ, first at {d[:6].tolist()}"
        assert not changes or len(xyz) == 0 or not sp.same_bytes(got[i], fields[i]), f"{what}: field {i}: nothing was added"
    d = np.flatnonzero(status != want_status)
    assert len(d) == 0, f"{what}: status differs at {d[:6].tolist()}: {status[d[:6]].tolist()} against {want_status[d[:6]].tolist()}"
    assert rej == want_rej, f"{what}: rejected {rej} against {want_rej}"
    return got


def prefix(c, n):
    return len(c["xyz"]) if n == "all" else n


# ---------------------------------------------------------------------------------------------------------------
# 1. the ordered call equals the mirror
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", bc.COUNTS)
@pytest.mark.parametrize("name", bc.GRIDS)
def test_ordered_splat_equals_the_mirror(name, n):
    R, c = rig(name), bc.case(name)  # (the conditions of the case: tests/test_splat_binned.py asserts them on the CPU)
    n = prefix(c, n)
    for label, (fields, values) in bc.channel_sets(name).items():  # float | Vec3f | 1 float + velocity (one pass) | 5 floats + velocity (two)
        for level in LEVELS:
            for rows in bc.ROWS:
                assert_equal_the_mirror(R, fields, c["xyz"][:n], [v[:n] for v in values], f"{name} n={n} {label} {level} {rows}", level=level, rows=rows)


@pytest.mark.parametrize("kind", LAUNCH_RANGES)
def test_every_leaf_is_summed_whatever_the_launch_range(kind):
    """include/hns.h: the order and the splat landing count every leaf whatever the grid's launch range, ghost leaves included -- sort and ordered splat under
    set_active_range on a strict inner range and under set_active_leaves(n // 2) give the bytes of the whole range, which equal the mirror"""
    R, c = rig("ragged32"), bc.case("ragged32")
    fields, values = bc.channel_sets("ragged32")["float+vec3"]
    for level in LEVELS:
        for rows in bc.ROWS:
            whole = assert_equal_the_mirror(R, fields, c["xyz"], values, f"whole range {level} {rows}", level=level, rows=rows)
            _, whole_status, whole_rejected = R.ordered(fields, c["xyz"], values, -32, level, rows, f"whole range {level} {rows}")
            with launch_range(R.grid, kind):
                got, status, rejected = R.ordered(fields, c["xyz"], values, -32, level, rows, f"{kind} {level} {rows}")
            assert R.grid.active_leaves() == R.grid.leaf_count()
            for i in range(len(fields)):
                assert sp.same_bytes(got[i], whole[i]), f"{kind} {level} {rows}: field {i} differs from the whole range's"
            assert np.array_equal(status, whole_status) and rejected == whole_rejected, f"{kind} {level} {rows}: status or rejected"


@pytest.mark.parametrize("radius", rc.RADII)
@pytest.mark.parametrize("name", bc.GRIDS)
def test_ordered_radial_splat_equals_the_mirror(name, radius):
    R, c = rig(name), bc.case(name, "radial")
    fields, values = bc.channel_sets(name, "radial")["float+vec3"]
    for level, rows in (("voxel", "original"), ("voxel", "ranked"), ("leaf", "original")):
        assert_equal_the_mirror(R, fields, c["xyz"], values, f"{name} r={radius} {level} {rows}", level=level, rows=rows, **rc.spec_of("radial", "add", radius))


@pytest.mark.parametrize("rows", bc.ROWS)
@pytest.mark.parametrize("name", bc.GRIDS)
def test_ordered_splat_with_one_radius_per_point_equals_the_mirror(name, rows):
    R, c = rig(name), bc.case(name, "radial")
    fields, values = bc.channel_sets(name, "radial")["5float+vec3"]  # two passes
    assert_equal_the_mirror(R, fields, c["xyz"], values, f"{name} per-point radii {rows}", rows=rows, radii=c["radii"], **rc.spec_of("radial", "add", 4.0))


@pytest.mark.parametrize("kernel,radius", (("trilinear", None), ("radial", 2.5)))
@pytest.mark.parametrize("name", bc.GRIDS)
def test_ordered_average_equals_the_mirror(name, kernel, radius):
    R, c = rig(name), bc.case(name, "radial")
    for label in ("float+vec3", "5float+vec3"):  # W + three channels: two passes | four passes, each with its own W
        fields, values = bc.channel_sets(name, "radial")[label]
        for rows in bc.ROWS:
            assert_equal_the_mirror(R, fields, c["xyz"], values, f"{name} average {kernel} {label} {rows}", rows=rows, **rc.spec_of(kernel, "average", radius, min_weight=0.25))


# ---------------------------------------------------------------------------------------------------------------
# 2. special values
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rows", bc.ROWS)
@pytest.mark.parametrize("level", LEVELS)
def test_special_values_equal_the_mirror(level, rows):
    """NaN, inf and out-of-range positions land nowhere (the tail); NaN, inf and out-of-bound values are counted and add nothing; five terms of 2^61 quanta wrap the
    accumulator in LDS as the mirror's wraps"""
    R, c = rig("ragged32"), bc.case("ragged32")
    xyz = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [3e9, 1, 1], [1, -3e9, 1], [1.5, 1.5, 1.5], [1.5, 1.5, 1.5], [1.5, 1.5, 1.5], [2, 2, 2], [2.25, 2.5, 2.5]]
                   + [[3.0, 3.0, 3.0]] * 5, dtype=F)
    vals = np.array([1, 1, 1, 1, 1, np.nan, np.inf, 2.0 ** 34, -np.inf, 2.0 ** 32] + [2.0 ** 29] * 5, dtype=F)
    fields, values = [c["phi"][0], c["vel"]], [vals, np.stack([vals, -vals, vals], 1)]
    got, status, rej = R.ordered(fields, xyz, values, -32, level, rows, "special values")
    want, want_status, want_rej = mirror(R, fields, xyz, values)
    assert sp.same_bytes(got[0], want[0]) and sp.same_bytes(got[1], want[1]) and sp.same_bytes(status, want_status)
    assert status.tolist() == [0] * 5 + [8] * 10 and rej == want_rej == 4 * 8 * 4


# ---------------------------------------------------------------------------------------------------------------
# 3. adversarial distributions
# ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def dense64_fields():
    rng = np.random.default_rng(97)
    N = len(oc.origins("dense64")) * 512
    phi, vel = rng.standard_normal(N).astype(F), rng.standard_normal((N, 3)).astype(F)
    vals, vvals = (rng.standard_normal(oc.N_BIG) * 3.0).astype(F), (rng.standard_normal((oc.N_BIG, 3)) * 3.0).astype(F)
    return phi, vel, vals, vvals


@pytest.mark.parametrize("kernel", ("trilinear", "radial"))
@pytest.mark.parametrize("kind", ("one_voxel", "corner_ball", "alternating", "all_outside", "all_nan", "reversed"))
def test_adversarial_distributions_equal_the_mirror(kind, kernel):
    """a leaf that takes every point, an emitter ball on a leaf corner, two far voxels in turn, a call that is all tail, a call where nothing lands, the reverse order"""
    R, xyz = rig("dense64"), oc.distribution(kind)
    phi, vel, vals, vvals = dense64_fields()
    spec = rc.spec_of("radial", "add", 1.5) if kernel == "radial" else {}
    nothing = kind == "all_nan"
    got = assert_equal_the_mirror(R, [phi, vel], xyz, [vals, vvals], f"{kind} {kernel}", changes=not nothing and kind != "all_outside", **spec)
    assert not nothing or (sp.same_bytes(got[0], phi) and sp.same_bytes(got[1], vel))


# ---------------------------------------------------------------------------------------------------------------
# 4. the accumulator between calls
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel", ("trilinear", "radial"))
def test_plain_and_ordered_calls_alternate_on_one_grid(kernel):
    """an ordered call leaves the accumulator and the touched words zero: a plain call of other points then equals the mirror of that call alone, and the other way round"""
    R, c = rig("ragged32"), bc.case("ragged32")
    spec = rc.spec_of("radial", "add", 2.5) if kernel == "radial" else {}
    half = len(c["xyz"]) // 2
    fields = [c["phi"][0], c["vel"]]
    a = (c["xyz"][:half], [c["vals"][0][:half], c["vvals"][:half]])  # (holds the planted pair: tail and leaf terms into one voxel)
    b = (c["xyz"][half:], [c["vals"][1][half:], c["vvals"][half:]])
    want_a, want_b = mirror(R, fields, *a, **spec)[0], mirror(R, fields, *b, **spec)[0]
    R.grid.release_cache()  # (whatever accumulator earlier tests left with the grid)
    first = R.ordered(fields, *a, what="ordered A", **spec)[0]
    plain_b = R.plain(fields, *b, **spec)
    ordered_a = R.ordered(fields, *a, what="ordered A after plain B", **spec)[0]
    plain_a = R.plain(fields, *a, **spec)
    ordered_b = R.ordered(fields, *b, what="ordered B after plain A", **spec)[0]
    for i in range(2):
        assert sp.same_bytes(first[i], want_a[i]), f"ordered A: field {i}"
        assert sp.same_bytes(plain_b[i], want_b[i]), f"plain B after ordered A: field {i}"
        assert sp.same_bytes(ordered_a[i], want_a[i]) and sp.same_bytes(ordered_a[i], first[i]), f"ordered A twice: field {i}"
        assert sp.same_bytes(plain_a[i], want_a[i]) and sp.same_bytes(ordered_b[i], want_b[i]), f"plain A, ordered B: field {i}"


# ---------------------------------------------------------------------------------------------------------------
# 5. the sim form
# ---------------------------------------------------------------------------------------------------------------

SIM_NAMES = ["density", "fuel", "collision_sdf"]


@pytest.mark.parametrize("kernel", ("trilinear", "radial"))
@pytest.mark.parametrize("activate", (True, False))
def test_sim_splat_through_an_order_equals_sim_splat(activate, kernel):
    import torch

    c = bc.case("ragged32")
    o, xyz, vals, vvals = c["o"], c["xyz"], c["vals"], c["vvals"]
    spec = rc.spec_of("radial", "add", 1.5) if kernel == "radial" else {}
    state = random_state(13, len(o), SIM_NAMES)
    (g, s), (g2, twin) = make_sim(o, SIM_NAMES, state, np.array(c["masks"]), VS), make_sim(o, SIM_NAMES, state, np.array(c["masks"]), VS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    p, values, vel = dev(xyz), {"fuel": dev(vals[0]), "density": dev(vals[1])}, dev(vvals)
    po = s.point_order(len(xyz)).sort(p)
    rej, rej2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    st = s.splat(values, p, velocity=vel, activate=activate, status=True, rejected=rej, order=po, **spec)
    want_st = twin.splat(values, p, velocity=vel, activate=activate, status=True, rejected=rej2, **spec)
    assert sp.same_bytes(st.cpu().numpy(), want_st.cpu().numpy()) and int(rej.cpu()[0]) == int(rej2.cpu()[0])
    # and on ranked rows, into the result
    ranked = {k: po.gather(v) for k, v in values.items()}
    st = s.splat(ranked, po.gather(p), velocity=po.gather(vel), activate=activate, status=True, order=po, rows="ranked", **spec)
    assert sp.same_bytes(po.scatter(st.view(torch.int8).to(torch.int32)).cpu().numpy(), want_st.to(torch.int32).cpu().numpy())
    twin.splat(values, p, velocity=vel, activate=activate, **spec)
    a, b = download(s, SIM_NAMES), download(twin, SIM_NAMES)
    for k in a:
        assert sp.same_bytes(a[k], b[k]), f"Sim.splat(order=...): {k}"
        assert k == "collision_sdf" or not sp.same_bytes(a[k], state[k])
    assert sp.same_bytes(s.active_masks(), twin.active_masks()) and sp.same_bytes(s.active_masks(), c["masks"]) == (not activate)
    po.close()

    # Sim.emit-style growth: after regrid(points=...) every tap of every seeding point lies inside, so the tail is empty and every status is 8
    seeds = dev(xyz[sd.seeding(xyz)])
    for sim in (s, twin):
        sim.regrid(1, points=seeds)
    po = s.point_order(len(seeds)).sort(seeds, "leaf")
    grown = {"density": dev(vals[2][: len(seeds)])}
    st = s.splat(grown, seeds, activate=activate, status=True, order=po)
    twin.splat(grown, seeds, activate=activate)
    ls = po.leaf_start.cpu().numpy().view(np.uint32)
    assert (st.cpu().numpy() == 8).all() and ls[s.grid.leaf_count()] == len(seeds), "after the regrid the tail is empty and every point lands whole"
    a, b = download(s, SIM_NAMES), download(twin, SIM_NAMES)
    for k in a:
        assert sp.same_bytes(a[k], b[k]), f"after regrid(points=...): {k}"
    assert sp.same_bytes(s.active_masks(), twin.active_masks())
    po.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. stream and pool
# ---------------------------------------------------------------------------------------------------------------


def test_sort_gather_and_splat_late_on_a_non_blocking_stream():
    """bound to a non-blocking stream, sort, gather and splat run behind a delay; xyz, the values and the field hold poison until their true values arrive on that stream"""
    import torch as t

    R = rig("dense64")
    xyz = oc.full_set("dense64")
    n = len(xyz)
    phi, _, vals, _ = dense64_fields()
    vals = vals[:n]
    want, want_status, _ = mirror(R, [phi], xyz, [vals])
    po = R.D.PointOrder(R.grid, n)
    x, v, f = R.dev(xyz), R.dev(vals), R.dev(phi)
    gx, gv = t.empty_like(x), t.empty_like(v)
    status = t.empty(n, dtype=t.uint8, device="cuda")

    def call(stream):
        po.sort(x, "voxel", stream=stream)
        po.gather(x, gx)
        po.gather(v, gv)
        po.splat([f], gx, [gv], status=status, rows="ranked")
        return {"perm": po.perm}

    t.cuda.synchronize()
    t0 = time.perf_counter()
    call(0)  # the null stream, device idle before and after: also loads the code objects
    host = time.perf_counter() - t0
    t.cuda.synchronize()
    assert sp.same_bytes(f.cpu().numpy(), want[0]), "null stream"
    delay = sc.Delay(t)
    late = sc.late_call(call, {"xyz": sc.Operand(x, R.dev(xyz)), "values": sc.Operand(v, R.dev(vals)), "field": sc.Operand(f, R.dev(phi))}, {"field": f, "status": status}, delay,
                        delay.for_host_time(host), what="ordered splat")
    assert late.armed_held
    assert sp.same_bytes(late.outputs["field"].cpu().numpy(), want[0]), "late stream: field"
    back = np.empty(n, dtype=np.uint8)
    back[late.outputs["perm"].cpu().numpy().view(np.uint32).astype(np.int64)] = late.outputs["status"].cpu().numpy()
    assert sp.same_bytes(back, want_status), "late stream: status"
    sc.assert_inputs_unchanged({k: late.inputs[k] for k in ("xyz", "values")}, {"xyz": xyz, "values": vals}, what="ordered splat")
    po.close()


@pytest.mark.parametrize("fill", (255, 127))
def test_nothing_depends_on_what_pooled_memory_held(fill):
    R, c = rig("ragged32_off_origin"), bc.case("ragged32_off_origin")
    fields, values = bc.channel_sets("ragged32_off_origin")["5float+vec3"]
    R.grid.release_cache()  # the accumulator and the order's buffers are drawn inside the block
    with arena_fill(fill):
        assert_equal_the_mirror(R, fields, c["xyz"], values, f"arena_fill {fill}")
    R.grid.release_cache()


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------


class Refusals:
    """one sim, one sorted order and the arrays of a call; every refusal must leave fields, status and d_rejected as they are"""

    def __init__(self):
        import torch

        from hnanosolver_amd import _lib, device

        self.torch, self.lib, self.BAD = torch, _lib.load_library(), _lib.HNS_ERR_INVALID_ARGUMENT
        c = bc.case("one_leaf")
        self.state, self.masks, self.n = random_state(3, len(c["o"]), SIM_NAMES), np.array(c["masks"]), 64
        self.g, self.s = make_sim(c["o"], SIM_NAMES, self.state, self.masks, VS)
        self.g2, self.s2 = make_sim(c["o"], SIM_NAMES, self.state, self.masks, VS)  # a sim on another grid
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.p, self.v, self.vv, self.field = dev(c["xyz"][: self.n]), dev(c["vals"][0][: self.n]), dev(c["vvals"][: self.n]), dev(self.state["density"])
        self.status = torch.full((self.n,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.rejected = torch.full((1,), REJECTED_BEFORE, dtype=torch.int64, device="cuda")
        self.po = device.PointOrder(self.g, self.n).sort(self.p)
        self.unsorted = device.PointOrder(self.g, self.n)

    P = staticmethod(lambda *ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]))
    N = staticmethod(lambda *names: (C.c_char_p * len(names))(*names))

    def grid_call(self, fields, nc, k, values, q=-32, x=None, rows=0, order=None):
        return self.lib.hns_point_order_splat(self.po._ptr if order is None else order, fields, (C.c_int * len(nc))(*nc), k, self.p.data_ptr() if x is None else x, values, rows, q,
                                              self.status.data_ptr(), self.rejected.data_ptr())

    def sim_call(self, names, k, velocity, values, q=-32, rows=0, order=None, sim=None):
        return self.lib.hns_point_order_splat_sim(self.po._ptr if order is None else order, self.s._ptr if sim is None else sim, names, k, velocity, self.p.data_ptr(), values, rows,
                                                  q, 1, self.status.data_ptr(), self.rejected.data_ptr())

    def check(self, call, code, word):
        text = self.lib.hns_last_error().decode()
        assert code == self.BAD and text.startswith(call + ":") and word in text, f"{call} (expects {word!r}): got {code} {text!r}"
        self.torch.cuda.synchronize()
        assert (self.status.cpu().numpy() == SENTINEL).all() and int(self.rejected.cpu()[0]) == REJECTED_BEFORE, f"{call} ({word}): status or d_rejected was written"
        assert sp.same_bytes(self.field.cpu().numpy(), self.state["density"]), f"{call} ({word}): the field was written"
        after = download(self.s, SIM_NAMES)
        assert all(sp.same_bytes(after[k], self.state[k]) for k in after) and sp.same_bytes(self.s.active_masks(), self.masks), f"{call} ({word}): the sim was written"


@functools.lru_cache(maxsize=None)
def refusals():
    return Refusals()


DEV, SIM = "hns_point_order_splat", "hns_point_order_splat_sim"
REFUSALS = {
    # what the plain calls refuse
    "two equal fields": (DEV, lambda r: r.grid_call(r.P(r.field, r.field), (1, 1), 2, r.P(r.v, r.v)), "fields[1] is fields[0]"),
    "a field that is a values array": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(r.field)), "fields[0] is values[0]"),
    "a field that is xyz": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(r.v), x=r.field.data_ptr()), "fields[0] is xyz"),
    "a field that is status": (DEV, lambda r: r.grid_call(r.P(r.status), (1,), 1, r.P(r.v)), "fields[0] is status"),
    "a field that is d_rejected": (DEV, lambda r: r.grid_call(r.P(r.rejected), (1,), 1, r.P(r.v)), "fields[0] is d_rejected"),
    "a null xyz": (DEV, lambda r: r.lib.hns_point_order_splat(r.po._ptr, r.P(r.field), (C.c_int * 1)(1), 1, None, r.P(r.v), 0, -32, r.status.data_ptr(), r.rejected.data_ptr()), "xyz is null"),
    "a null field": (DEV, lambda r: r.grid_call(r.P(None), (1,), 1, r.P(r.v)), "fields[0] is null"),
    "a null values entry": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(None)), "values[0] is null"),
    "a null list": (DEV, lambda r: r.grid_call(None, (1,), 1, r.P(r.v)), "null list"),
    "an ncomp of 2": (DEV, lambda r: r.grid_call(r.P(r.field), (2,), 1, r.P(r.v)), "ncomp[0] is 2"),
    "nine fields": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 9, r.P(r.v)), "n_fields is 9"),
    "a positive log2_quantum": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(r.v), 1), "log2_quantum is 1"),
    "an unknown name": (SIM, lambda r: r.sim_call(r.N(b"smoke"), 1, None, r.P(r.v)), "no float field named 'smoke'"),
    "a name twice": (SIM, lambda r: r.sim_call(r.N(b"density", b"density"), 2, None, r.P(r.v, r.v)), "listed twice"),
    "collision_sdf": (SIM, lambda r: r.sim_call(r.N(b"collision_sdf"), 1, None, r.P(r.v)), "collision_sdf"),
    "nothing to write": (SIM, lambda r: r.sim_call(None, 0, None, None), "nothing to write"),
    "a log2_quantum of -41": (SIM, lambda r: r.sim_call(r.N(b"density"), 1, r.vv.data_ptr(), r.P(r.v), -41), "log2_quantum is -41"),
    "a null sim values entry": (SIM, lambda r: r.sim_call(r.N(b"density"), 1, None, r.P(None)), "values[0] is null"),
    "a null sim": (SIM, lambda r: r.lib.hns_point_order_splat_sim(r.po._ptr, None, r.N(b"density"), 1, None, r.p.data_ptr(), r.P(r.v), 0, -32, 1, r.status.data_ptr(), r.rejected.data_ptr()),
                   "null sim"),
    # and what is the ordered calls' own
    "a null object": (DEV, lambda r: r.lib.hns_point_order_splat(None, r.P(r.field), (C.c_int * 1)(1), 1, r.p.data_ptr(), r.P(r.v), 0, -32, r.status.data_ptr(), r.rejected.data_ptr()),
                      "null point order"),
    "a null object, sim form": (SIM, lambda r: r.lib.hns_point_order_splat_sim(None, r.s._ptr, r.N(b"density"), 1, None, r.p.data_ptr(), r.P(r.v), 0, -32, 1, r.status.data_ptr(),
                                                                                  r.rejected.data_ptr()), "null point order"),
    "a call before any sort": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(r.v), order=r.unsorted._ptr), "no sort has run"),
    "a call before any sort, sim form": (SIM, lambda r: r.sim_call(r.N(b"density"), 1, None, r.P(r.v), order=r.unsorted._ptr), "no sort has run"),
    "rows of 2": (DEV, lambda r: r.grid_call(r.P(r.field), (1,), 1, r.P(r.v), rows=2), "rows is 2"),
    "rows of -1, sim form": (SIM, lambda r: r.sim_call(r.N(b"density"), 1, None, r.P(r.v), rows=-1), "rows is -1"),
    "a sim on another grid": (SIM, lambda r: r.sim_call(r.N(b"density"), 1, None, r.P(r.v), sim=r.s2._ptr), "the sim's grid is not the grid of the point order"),
}


@pytest.mark.parametrize("item", sorted(REFUSALS))
def test_refused_before_anything_is_launched(item):
    call, fn, word = REFUSALS[item]
    r = refusals()
    r.check(call, fn(r), word)


def test_no_points_launch_nothing_and_look_at_no_device_pointer():
    from hnanosolver_amd import _lib

    R, lib = rig("one_leaf"), _lib.load_library()
    po = R.D.PointOrder(R.grid, 4).sort(R.t.zeros((0, 3), device="cuda"))
    bogus = (C.c_void_p * 2)(0x10, None)
    assert lib.hns_point_order_splat(po._ptr, bogus, (C.c_int * 2)(1, 3), 2, None, bogus, 1, -32, 0x10, 0x10) == 0
    R.t.cuda.synchronize()
    po.close()
