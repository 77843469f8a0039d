"""TEST HELPER of tests/test_stream_cases.py (CPU) and tests/test_streams_gpu.py: every entry point of include/hns.h that takes a `void* stream`, run LATE on a
non-blocking stream and inside guard bands.

What the rest of the suite cannot see is ordering and write extent: nearly every GPU test calls the library on the legacy null stream, which the runtime serialises
against everything, and allocates each output on its own. Here

  late_call   runs one call on a non-blocking stream S on which the true inputs arrive only behind a delay: until then the inputs hold NaN (index and mask inputs a
              valid but different value, so nothing can address out of range) and the outputs a sentinel. Whatever part of the call is not ordered behind S -- a
              launch, memset or copy on another stream, a forgotten event -- reads the poison or is overwritten by the sentinel, and the bytes come out wrong.
  Slab        carves the outputs out of one patterned buffer with two leaves of the widest field (2 x 512 x 3 x 4 B) between and around them; check() finds any store
              outside an output. Every view is 256-byte aligned unless it is given a skew: tests/layout_cases.py starts views 1 .. 12 bytes behind that, the least
              alignment include/hns.h asks of a device operand.
              Guard bands cover the KERNEL level (hns_dev_*), where the caller owns every output. At sim level the fields belong to the library and the point
              outputs (sampled values, status, moved positions) are allocated by device.Sim; they are compared, not guard-banded.
  CASES       entry point -> (level, source of the expected bytes, variants). The coverage test in tests/test_stream_cases.py fails for an entry point with a stream
              parameter that is neither here nor in EXEMPT.

Expected bytes come from the CPU oracle (oracle_lib.OracleGrid) or a host mirror where the suite has one for the call ("oracle" / "mirror" below), and ALWAYS from the
same call on the null stream with the device idle before and after ("null stream"): the late run must equal both. The null-stream run is also where the host time of
the call is taken; the delay in front of the late run is at least ten times that (and at least MIN_DELAY_MS).

Measured on an MI355X (HOST_TIMES, printed by tests/test_streams_gpu.py::test_report), 91 cases: one delay operation (add_ over 2^25 floats) is 37.8 us of GPU time.
Host time of the null-stream call: 21 us (pack_leaves) to 31 ms, median 68 us. Kernel-level calls 21 - 160 us, median 48 us, except the first call of a kind in the
process, which loads code objects and builds launch tables (advect_vector 8.5 ms, sample_points 1.9 ms, the first 4-iteration SOR launches 0.7 - 1.1 ms, divergence
and combustion 0.9 ms, splat 0.7 ms); sim-level asynchronous calls 44 - 180 us (upload 61 us, substep 135 - 181 us, two core substeps 125 - 135 us; deactivate 1.1 ms with
its first mask allocation); synchronous ones 0.28 - 4 ms (active_masks 0.28, stats 0.35, download 0.64, controlled solve 0.5 - 0.7, the regrids 4 ms, the first of them
31 ms). Delay enqueued: 2.0 ms, the floor, for the 70 cases under 200 us; ten times the host time for the rest: 2.8 - 40 ms, 85 ms for the first advect_vector and
314 ms for the first regrid. `armed` held in every asynchronous case.
"""
from __future__ import annotations

import math
import time
from collections import namedtuple

import numpy as np

F = np.float32
NAN_WORD = 0x7FC0DEAD    # float inputs before their true values arrive: a quiet NaN one recognises in a dump
OUT_WORD = 0xDEADBEEF    # outputs before the call
OUT_BYTE = 0xAB          # byte outputs before the call
GUARD_WORD = 0x6B8B4567  # the slab's pattern
ALIGN = 256
GUARD_BYTES = 2 * 512 * 3 * 4  # two leaves of a Vec3f field; a multiple of ALIGN
MIN_DELAY_MS = 2.0
DELAY_FACTOR = 10.0
assert GUARD_BYTES % ALIGN == 0

HOST_TIMES = {}  # case id -> (host seconds of the null-stream call, milliseconds of delay enqueued in front of the late one)


class NS(dict):
    """a dict read with attributes; a missing name reads None"""

    def __getattr__(self, k):
        return self.get(k)


def _signed(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def fill_words(t, word):
    """every 32-bit word of tensor t := word (every byte of a uint8 tensor := its low byte), on the current stream"""
    import torch

    if t.dtype == torch.uint8:
        t.fill_(word & 0xFF)
    else:
        t.view(torch.int32).fill_(_signed(word))


def sentinel(t):
    """an output before the call: OUT_WORD in every word, OUT_BYTE in every byte of a byte output"""
    import torch

    fill_words(t, OUT_BYTE if t.dtype == torch.uint8 else OUT_WORD)


def words(a) -> np.ndarray:
    """the raw bytes of a numpy array or tensor, as a flat uint8 array (NaN compares by bit pattern)"""
    if not isinstance(a, np.ndarray):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_words(a, b) -> bool:
    a, b = words(a), words(b)
    return a.size == b.size and bool(np.array_equal(a, b))


def _torch_dtype(torch, dtype):
    return getattr(torch, np.dtype(dtype).name)  # float32, int32, uint8, int64: the same names


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------


class Slab:
    """One uint32 tensor filled with GUARD_WORD from which buffers are carved as views, each with at least GUARD_BYTES of pattern on both sides and 256-byte aligned --
    or, with a skew, starting that many bytes behind a multiple of 256: the skipped bytes are guard like the rest."""

    def __init__(self, torch, specs, device="cpu", skew=None):
        """specs: {name: (shape, numpy dtype)} -> self.views[name]; skew: None, or {name: bytes in 0 .. 255, a multiple of the element size} (a name left out: 0)"""
        self.torch = torch
        assert not set(skew or {}) - set(specs), "a skew for a view that is not in specs"
        skew = {k: int((skew or {}).get(k, 0)) for k in specs}
        assert all(0 <= b < ALIGN and b % np.dtype(specs[k][1]).itemsize == 0 for k, b in skew.items()), skew
        total = GUARD_BYTES + sum(self._padded(skew[k] + self._nbytes(s, d)) + GUARD_BYTES for k, (s, d) in specs.items())
        self._store = torch.empty(total // 4, dtype=torch.int32, device=device)
        self._store.fill_(_signed(GUARD_WORD))
        self.words = self._store.view(torch.uint32) if hasattr(torch, "uint32") else self._store
        self.bytes = self._store.view(torch.uint8)
        if self._store.is_cuda:
            assert self._store.data_ptr() % ALIGN == 0
        self.extents, self.views, cursor = [], NS(), GUARD_BYTES
        for name, (shape, dtype) in specs.items():
            n, start = self._nbytes(shape, dtype), cursor + skew[name]
            self.views[name] = self.bytes[start:start + n].view(_torch_dtype(torch, dtype)).reshape(shape)
            self.extents.append((name, start, n))
            cursor += self._padded(skew[name] + n) + GUARD_BYTES
        assert cursor == total

    @staticmethod
    def _nbytes(shape, dtype):
        return int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize

    @staticmethod
    def _padded(n):
        return -(-n // ALIGN) * ALIGN

    def check(self, what=""):
        """asserts that every byte outside the carved views still holds the pattern; the message names the guard and the first byte hit"""
        host = self.bytes.cpu().numpy()
        pattern = np.full(host.size // 4, GUARD_WORD, dtype="<u4").view(np.uint8)
        guard = np.ones(host.size, dtype=bool)
        for _, start, n in self.extents:
            guard[start:start + n] = False
        bad = np.flatnonzero(guard & (host != pattern))
        if bad.size == 0:
            return
        b = int(bad[0])
        where = []
        for name, start, n in self.extents:
            if b >= start + n:
                where = [f"trailing guard of {name}, {b - start - n} bytes past its end"]  # (the nearest view in front)
            elif b < start:
                where.append(f"leading guard of {name}, {start - b} bytes before its start")
                break
        where = "; ".join(where)
        raise AssertionError(f"{what}: {bad.size} guard bytes overwritten, the first at slab byte {b} ({where}): 0x{host[b]:02x}")


def assert_inputs_unchanged(after, staging, inplace=(), what=""):
    """after, staging: {name: tensor or array}; every operand outside `inplace` (the operands documented as in-place) must hold its staging copy word for word"""
    for name, s in staging.items():
        if name in inplace:
            continue
        a, b = words(after[name]), words(s)
        if a.size != b.size or not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0]) if a.size == b.size else -1
            raise AssertionError(f"{what}: input {name} was written by the call (first changed byte {i})")


# ---------------------------------------------------------------------------------------------------------------------
# the late call
# ---------------------------------------------------------------------------------------------------------------------


class Delay:
    """GPU time in front of a call: plain elementwise torch operations on a large scratch tensor, timed once with events"""

    def __init__(self, torch, floats=1 << 25):
        self.torch = torch
        self.scratch = torch.zeros(floats, device="cuda")
        for _ in range(8):  # (loads the kernel)
            self.scratch.add_(1.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(64):
            self.scratch.add_(1.0)
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_op = e0.elapsed_time(e1) / 64.0

    def for_host_time(self, host_seconds):
        return max(MIN_DELAY_MS, DELAY_FACTOR * host_seconds * 1e3)

    def enqueue(self, ms):
        """on the current stream; returns the milliseconds enqueued"""
        n = max(1, math.ceil(ms / self.ms_per_op))
        for _ in range(n):
            self.scratch.add_(1.0)
        return n * self.ms_per_op


class Operand:
    """a tensor the call reads: its true values wait in `staging`; until they arrive it holds `poison` (None: NAN_WORD in every word)"""

    def __init__(self, tensor, staging, poison=None):
        self.tensor, self.staging, self.poison = tensor, staging, poison

    def spoil(self):
        if self.poison is None:
            fill_words(self.tensor, NAN_WORD)
        else:
            self.tensor.copy_(self.poison, non_blocking=True)

    def arrive(self):
        self.tensor.copy_(self.staging, non_blocking=True)


Late = namedtuple("Late", "outputs inputs returned armed_held delay_ms")


class LateRun:
    """late_call in three steps, so that two runs can be in flight at once: prepare() both, launch() both, finish() both.
    call_stream: the stream the call goes to when it is NOT the one the inputs arrive on -- the ordering bug tests/test_streams_gpu.py plants to see the harness bite."""

    def __init__(self, fn, inputs, outputs, delay, delay_ms, stream=None, call_stream=None):
        import torch

        self.torch, self.fn, self.inputs, self.outputs, self.delay, self.delay_ms = torch, fn, inputs, outputs, delay, delay_ms
        self.S = stream or torch.cuda.Stream()  # non-blocking: nothing orders it against the null stream
        self.C = call_stream or self.S
        self.armed = torch.cuda.Event()

    def _sentinels(self):
        for name, t in self.outputs.items():
            if name not in self.inputs:
                sentinel(t)

    def prepare(self):
        torch = self.torch
        torch.cuda.synchronize()  # 1. the device idle: poison everywhere
        for op in self.inputs.values():
            op.spoil()
        self._sentinels()
        torch.cuda.synchronize()
        return self

    def launch(self):
        torch = self.torch
        with torch.cuda.stream(self.S):  # 2.
            self.used = self.delay.enqueue(self.delay_ms)
            self.armed.record(self.S)
            for op in self.inputs.values():  # 3. the true inputs, behind the delay
                op.arrive()
            self._sentinels()  # (the sentinel once more: a store of the call that ran ahead of S is overwritten here)
        with torch.cuda.stream(self.C):
            self.returned = self.fn(stream=int(self.C.cuda_stream))  # 4.
            self.held = not self.armed.query()  # 5.
            extra = self.returned if isinstance(self.returned, dict) else {}
            self.got = {k: t.clone() for k, t in {**self.outputs, **{k: v for k, v in extra.items() if torch.is_tensor(v)}}.items()}  # 6.
            self.seen = {k: op.tensor.clone() for k, op in self.inputs.items()}
            for op in self.inputs.values():
                op.spoil()
        return self

    def finish(self, asynchronous=True, what=""):
        self.C.synchronize()  # 7. (everything above is still referenced here: the caching allocator knows nothing about S)
        self.S.synchronize()
        if asynchronous:
            assert self.held, f"{what}: the {self.used:.2f} ms delay had drained when the call returned; the inputs were no longer late and the case tested nothing"
        return Late(self.got, self.seen, self.returned, self.held, self.used)


def late_call(fn, inputs, outputs, delay, delay_ms, asynchronous=True, stream=None, what=""):
    """fn(stream=<hipStream_t as int>) on a non-blocking stream on which the true inputs arrive behind a delay.
    inputs: {name: Operand}; outputs: {name: tensor} (an in-place operand is in both). Tensors in a dict that fn returns are outputs too.
    -> Late(clones of the outputs, clones of the inputs as the call left them, what fn returned, ...). Raises if an asynchronous call returned only after the delay
    had drained: such a run tested nothing."""
    return LateRun(fn, inputs, outputs, delay, delay_ms, stream).prepare().launch().finish(asynchronous, what)


# ---------------------------------------------------------------------------------------------------------------------
# grids and fields
# ---------------------------------------------------------------------------------------------------------------------


def scattered_leaves():
    """the ~450-leaf lattice of tests/test_kernel_variants_gpu.py: 45 % of a 10^3 lattice, negative coordinates, ragged z-runs, lone leaves"""
    from hnanosolver_amd import fields

    rng = np.random.default_rng(77)
    lat = np.stack(np.meshgrid(*[np.arange(-5, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    scat = (lat[rng.random(len(lat)) < 0.45] * 8).astype(np.int32)
    return np.ascontiguousarray(scat[fields.nanovdb_order(scat)])


def mirrored_leaves():
    """scattered_leaves mirrored through the point (-4, -4, -4): another topology with the same leaf count, so its tables fit the memory the first one's leave behind"""
    from hnanosolver_amd import fields

    o = (-scattered_leaves() - 8).astype(np.int32)
    return np.ascontiguousarray(o[fields.nanovdb_order(o)])


def plume_leaves():
    from hnanosolver_amd import fields

    return fields.plume_leaves(8, 1.0, 0.3)


GRIDS = {"scattered": (scattered_leaves, 80), "plume": (plume_leaves, 64), "mirrored": (mirrored_leaves, 80)}  # (mirrored: the pool test's second owner only)
SIM_NAMES = ["density", "fuel", "waste", "temperature", "flame", "collision_sdf"]
N_POINTS = 1031  # no multiple of a wave or a workgroup


def noisy_fields(origins, R, amplitude, seed):
    """tests/test_parity_gpu.py's fields: the smooth synthetic ones plus 5 % noise, so no value is a signed zero and the advection kernels match the oracle bit for bit"""
    from hnanosolver_amd import fields

    f = fields.synthetic_fields(origins, R, amplitude_voxels=amplitude)
    rng = np.random.default_rng(seed)
    for k in f:
        f[k] = (f[k] + 0.05 * rng.standard_normal(f[k].shape) * max(1e-3, np.abs(f[k]).max())).astype(F)
    return f


class Ctx:
    """one grid with everything the cases read: computed once, never written"""

    def __init__(self, name):
        from hnanosolver_amd import fields
        from oracle_lib import OracleGrid, oracle
        from points_cases import make_points

        make, self.R = GRIDS[name]
        self.name, self.origins = name, make()
        self.nl, self.N = len(self.origins), len(self.origins) * 512
        self.vs = 1.0 / self.R
        self.inv_dx = float(F(1.0) / F(self.vs))
        self.dt = float(F(1.0 / 24.0))
        self.far = noisy_fields(self.origins, self.R, 400.0, 1)   # back-traces of ~17 voxels: far taps go through the origin hash
        self.f = noisy_fields(self.origins, self.R, 160.0, 2)
        sdf = fields.sphere_sdf(self.origins, self.R, center=(0.5, 0.3, 0.5), radius=0.2)
        sdf[::7] = F(0.05)  # the thin 0 <= sdf < 0.1 band
        self.sdf = sdf
        rng = np.random.default_rng(3)
        self.p = rng.standard_normal(self.N).astype(F)
        self.p_small = (0.01 * rng.standard_normal(self.N)).astype(F)
        self.oracle = OracleGrid(self.origins)
        self.omega = float(oracle().orc_omega_compute(self.vs))
        self.div = self.oracle.divergence(self.f["vel"], self.inv_dx)
        self.xyz = make_points(self.origins, 5, N_POINTS)
        self.values = rng.standard_normal(N_POINTS).astype(F)
        self.values3 = rng.standard_normal((N_POINTS, 3)).astype(F)
        self.masks = np.packbits(rng.random((self.nl, 64, 8)) < 0.6, axis=2, bitorder="little").reshape(self.nl, 64)
        self.ids = rng.permutation(self.nl)[: max(1, self.nl // 2)].astype(np.int32)
        self.state = {k: self.f[k] for k in ("vel", "density", "fuel", "waste", "temperature", "flame")}
        self.state["collision_sdf"] = self.sdf
        for a in [self.sdf, self.p, self.p_small, self.div, self.xyz, self.values, self.values3, self.masks, self.ids, *self.far.values(), *self.f.values()]:
            a.setflags(write=False)
        self.far_state = dict(self.state, **self.far)
        self._grid, self._pinned = None, {}

    @property
    def grid(self):
        if self._grid is None:
            from hnanosolver_amd import api

            self._grid = api.create_grid_from_leaves(self.origins, self.vs)
        return self._grid

    def with_fresh_grid(self):
        """the same data on a grid handle of its own, made at its first use"""
        import copy

        y = copy.copy(self)
        y._grid = None
        return y

    def pinned_state(self, which="state"):
        """the sim's state (which = "far_state": the fields of the long back-traces) in pinned host memory, so that hns_sim_upload's copies are asynchronous: {name: numpy view}"""
        if which not in self._pinned:
            import torch

            keep = {k: torch.from_numpy(np.array(v)).pin_memory() for k, v in getattr(self, which).items()}
            self._pinned[which] = (keep, {k: t.numpy() for k, t in keep.items()})
        return self._pinned[which][1]


# ---------------------------------------------------------------------------------------------------------------------
# kernel-level cases: hns_dev_* on caller-owned device memory
# ---------------------------------------------------------------------------------------------------------------------


class Call:
    """One kernel-level case on a Ctx.
    inputs   {name: array}: what the call reads; an in-place operand is listed here and in `inplace`
    poison   {name: array}: for index, id, count and mask inputs the valid but different value they hold until the true one arrives (float inputs hold NaN)
    outputs  {name: (shape, dtype)}: carved from the Slab together with the in-place operands
    run(t)   the library call(s) on the current stream, t = NS of device tensors by name; may return a tensor or a dict of tensors (further outputs)
    expect(h) None, or h = NS of the true inputs -> {output name: array} from the oracle or a host mirror
    """

    def __init__(self, inputs, outputs, run, expect=None, inplace=(), poison=None, asynchronous=True, options=None):
        self.inputs, self.outputs, self.run, self.expect = inputs, outputs, run, expect
        self.inplace, self.poison, self.asynchronous, self.options = tuple(inplace), poison or {}, asynchronous, options or {}


class Bench:
    """the device side of a Call: the slab, the tensors, the staging copies"""

    def __init__(self, torch, call, shorten=None):
        self.torch, self.call = torch, call
        specs = {k: (call.inputs[k].shape, call.inputs[k].dtype) for k in call.inplace}
        specs.update(call.outputs)
        self.slab = Slab(torch, specs, "cuda")
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases' arrays are read-only)
        self.staging = {k: dev(v) for k, v in call.inputs.items()}
        self.t = NS({k: (self.slab.views[k] if k in call.inplace else torch.empty_like(self.staging[k])) for k in call.inputs})
        self.t.update({k: self.slab.views[k] for k in call.outputs})
        self.operands = {k: Operand(self.t[k], self.staging[k], dev(call.poison[k]) if k in call.poison else None) for k in call.inputs}
        self.outputs = {k: self.t[k] for k in list(call.inplace) + list(call.outputs)}

    def on_null_stream(self):
        """the same call with the device idle before and after -> ({output: array}, {input: array as the call left it}, host seconds of the call)"""
        torch = self.torch
        for op in self.operands.values():
            op.arrive()
        for k in self.call.outputs:
            sentinel(self.t[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = self.call.run(self.t)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        extra = r if isinstance(r, dict) else {}  # (the device module hands its output tensor back: already an output here)
        got = {k: v.cpu().numpy().copy() for k, v in {**self.outputs, **extra}.items()}
        return got, {k: op.tensor.cpu().numpy().copy() for k, op in self.operands.items()}, host

    def late_run(self, delay, delay_ms, stream=None, call_stream=None):
        def fn(stream):
            from hnanosolver_amd import device as D

            assert D.current_stream() == stream
            r = self.call.run(self.t)
            return r if isinstance(r, dict) else None

        return LateRun(fn, self.operands, self.outputs, delay, delay_ms, stream, call_stream)

    def late(self, delay, delay_ms, what, asynchronous=None):
        return self.late_run(delay, delay_ms).prepare().launch().finish(self.call.asynchronous if asynchronous is None else asynchronous, what)


def assert_same_outputs(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        if not same_words(got[k], want[k]):
            a, b = words(got[k]), words(want[k])
            n = int((a != b).sum()) if a.size == b.size else -1
            raise AssertionError(f"{what}: output {k} differs in {n} of {b.size} bytes")


def check_call(torch, call, delay, what):
    """null-stream run, oracle / mirror, late run, guards, inputs -> the Late record"""
    import hnanosolver_amd as H

    try:
        for k, v in call.options.items():
            H.set_option(k, v)
        b = Bench(torch, call)
        ref, ref_inputs, host = b.on_null_stream()
        b.slab.check(f"{what}, null stream")
        assert_inputs_unchanged(ref_inputs, call.inputs, call.inplace, f"{what}, null stream")
        h = NS(call.inputs)
        if call.expect is not None:
            for k, v in call.expect(h).items():
                assert same_words(ref[k], v), f"{what}: output {k} on the null stream differs from the oracle / host mirror"
        ms = delay.for_host_time(host)
        late = b.late(delay, ms, what)
        HOST_TIMES[what] = (host, late.delay_ms)
        assert_same_outputs(late.outputs, ref, f"{what}, late on a non-blocking stream")
        b.slab.check(f"{what}, late")
        assert_inputs_unchanged(late.inputs, call.inputs, call.inplace, f"{what}, late")
        return late, ref
    finally:
        for k in call.options:
            H.set_option(k, None)


def _D():
    from hnanosolver_amd import device

    return device


def _vec(x):
    return ((x.N, 3), F)


def _flt(x):
    return ((x.N,), F)


def k_advect_vector(coll):
    def build(x):
        ins = {"vel": x.far["vel"], **({"sdf": x.sdf} if coll else {})}
        return Call(ins, {"out": _vec(x)}, lambda t: _D().advect_vector(x.grid, t.vel, t.out, x.dt, x.inv_dx, t.sdf, coll),
                    lambda h: {"out": x.oracle.advect_vector(h.vel, x.dt, x.inv_dx, h.sdf, coll)})
    return build


def k_advect_scalar(coll):
    def build(x):
        ins = {"vel": x.far["vel"], "phi": x.far["density"], **({"sdf": x.sdf} if coll else {})}
        return Call(ins, {"out": _flt(x)}, lambda t: _D().advect_scalar(x.grid, t.vel, t.phi, t.out, x.dt, x.inv_dx, t.sdf, coll),
                    lambda h: {"out": x.oracle.advect_scalar(h.vel, h.phi, x.dt, x.inv_dx, h.sdf, coll)})
    return build


def _many(x, names, coll, fn, oracle_fn):
    ins = {"vel": x.far["vel"], **{n: x.far[n] for n in names}, **({"sdf": x.sdf} if coll else {})}
    outs = {f"out_{n}": _flt(x) for n in names}
    run = lambda t: fn(x.grid, t.vel, [t[n] for n in names], [t[f"out_{n}"] for n in names], x.dt, x.inv_dx, t.sdf, coll)
    return Call(ins, outs, run, lambda h: dict(zip(outs, oracle_fn(h))))


def k_advect_scalars(coll):
    names = ("density", "fuel") if coll else ("density", "temperature", "fuel", "waste", "flame")
    return lambda x: _many(x, names, coll, _D().advect_scalars, lambda h: x.oracle.advect_scalars(h.vel, [h[n] for n in names], x.dt, x.inv_dx, h.sdf, coll))


def k_advect_scalar_multi(coll):
    names = ("density", "temperature", "fuel")
    return lambda x: _many(x, names, coll, _D().advect_scalar_multi, lambda h: [x.oracle.advect_scalar(h.vel, h[n], x.dt, x.inv_dx, h.sdf, coll) for n in names])


def k_advect_scalars_ahead(x):
    names = ("density", "temperature", "fuel")
    ins = {"vel": x.far["vel"], **{n: x.far[n] for n in names}}
    outs = {**{f"out_{n}": _flt(x) for n in names}, "adv": _vec(x)}
    run = lambda t: _D().advect_scalars_ahead(x.grid, t.vel, [t[n] for n in names], [t[f"out_{n}"] for n in names], t.adv, x.dt, x.inv_dx)
    expect = lambda h: {**dict(zip(outs, x.oracle.advect_scalars(h.vel, [h[n] for n in names], x.dt, x.inv_dx))), "adv": x.oracle.advect_vector(h.vel, x.dt, x.inv_dx)}
    return Call(ins, outs, run, expect)


def k_divergence(x):
    return Call({"vel": x.f["vel"]}, {"div": _flt(x)}, lambda t: _D().divergence(x.grid, t.vel, t.div, x.inv_dx),
                lambda h: {"div": x.oracle.divergence(h.vel, x.inv_dx)})


def k_rbgs_color(x):
    def run(t):
        for color in (0, 1, 0):
            _D().rbgs_color(x.grid, t.div, t.p, x.vs, x.omega, color)

    def expect(h):
        p = np.array(h.p)
        for color in (0, 1, 0):
            x.oracle.rbgs(h.div, p, x.vs, color, x.omega)
        return {"p": p}

    return Call({"div": x.div, "p": x.p_small}, {}, run, expect, inplace=("p",))


def k_rbgs_iterate(options, iterations):
    """p_a holds a non-zero start, so every tap matters; both buffers are the call's to write. The result (p_a or p_b, by *result_in_b) against the oracle"""
    def build(x):
        run = lambda t: {"result": _D().rbgs_iterate(x.grid, t.div, t.p_a, t.p_b, x.vs, x.omega, iterations)}
        expect = lambda h: {"result": x.oracle.rbgs_iterations(h.div, x.vs, x.omega, iterations, h.p_a)}
        return Call({"div": x.div, "p_a": x.p_small, "p_b": np.zeros(x.N, F)}, {}, run, expect, inplace=("p_a", "p_b"), options=options)
    return build


def k_gradient(coll):
    def build(x):
        ins = {"vel": x.f["vel"], "p": x.p, **({"sdf": x.sdf} if coll else {})}
        return Call(ins, {"out": _vec(x)}, lambda t: _D().subtract_pressure_gradient(x.grid, t.vel, t.p, t.out, x.inv_dx, t.sdf, coll),
                    lambda h: {"out": x.oracle.subtract_pressure_gradient(h.vel, h.p, x.inv_dx, h.sdf, coll)})
    return build


def k_combustion(x):
    names = ("fuel", "waste", "temperature", "flame")
    waste = (0.5 * np.abs(np.random.default_rng(8).standard_normal(x.N))).astype(F)  # some voxels end with oxygen < 0
    ins = {"fuel": x.f["fuel"], "waste": waste, "temperature": x.f["temperature"], "div": x.div, "flame": x.f["flame"]}
    outs = {f"out_{n}": _flt(x) for n in names}
    run = lambda t: _D().combustion_oxygen(t.fuel, t.waste, t.temperature, t.div, t.flame, *[t[k] for k in outs], 0.5, 0.1)
    expect = lambda h: dict(zip(list(outs) + ["div"], x.oracle.combustion_oxygen(h.fuel, h.waste, h.temperature, h.div, h.flame, 0.5, 0.1)))
    return Call(ins, outs, run, expect, inplace=("div",))


def k_buoyancy(x):
    return Call({"vel": x.f["vel"], "temperature": x.f["temperature"]}, {"out": _vec(x)},
                lambda t: _D().temperature_buoyancy(t.vel, t.temperature, t.out, x.dt, 23.0, 1.0),
                lambda h: {"out": x.oracle.temperature_buoyancy(h.vel, h.temperature, x.dt, 23.0, 1.0)})


def k_vorticity(factor_scale):
    return lambda x: Call({"vel": x.f["vel"]}, {"out": _vec(x)}, lambda t: _D().vorticity_confinement(x.grid, t.vel, t.out, x.dt, x.inv_dx, 1.0, factor_scale),
                          lambda h: {"out": x.oracle.vorticity_confinement(h.vel, x.dt, x.inv_dx, 1.0, factor_scale)})


def k_enforce(x):
    return Call({"vel": x.f["vel"], "sdf": x.sdf}, {}, lambda t: _D().enforce_collision_boundaries(x.grid, t.vel, t.sdf, x.vs),
                lambda h: {"vel": x.oracle.enforce_collision_boundaries(h.vel, h.sdf, x.vs)}, inplace=("vel",))


def k_pack(ncomp):
    def build(x):
        field = x.f["vel"] if ncomp == 3 else x.f["density"]
        n = len(x.ids)
        expect = lambda h: {"packed": np.ascontiguousarray(np.asarray(h.field).reshape(x.nl, 512 * ncomp)[h.ids].reshape(-1))}
        return Call({"field": field, "ids": x.ids}, {"packed": ((n * 512 * ncomp,), F)}, lambda t: _D().pack_leaves(t.field, t.ids, t.packed, ncomp), expect,
                    poison={"ids": np.ascontiguousarray(x.ids[::-1])})  # a valid but different list: the same leaves in reverse
    return build


def k_unpack(ncomp):
    def build(x):
        n = len(x.ids)
        packed = np.random.default_rng(12).standard_normal(n * 512 * ncomp).astype(F)

        def expect(h):
            out = np.full((x.nl, 512 * ncomp), OUT_WORD, dtype=np.uint32)  # the leaves not listed keep the sentinel
            out[h.ids] = np.asarray(h.packed).view(np.uint32).reshape(n, 512 * ncomp)
            return {"field": out.reshape(-1)}

        return Call({"packed": packed, "ids": x.ids}, {"field": _vec(x) if ncomp == 3 else _flt(x)}, lambda t: _D().unpack_leaves(t.packed, t.ids, t.field, ncomp),
                    expect, poison={"ids": np.ascontiguousarray(x.ids[::-1])})
    return build


def k_sample_points(x):
    n = N_POINTS

    def expect(h):
        from points_cases import fma_branch

        with fma_branch(x.oracle.L):  # the Vec3f lerp the advection kernels are pinned to
            v = x.oracle.sample_trilinear_v(h.vel, h.xyz)
        return {"out_density": x.oracle.sample_trilinear_f(h.density, h.xyz), "out_vel": v, "out_fuel": x.oracle.sample_trilinear_f(h.fuel, h.xyz)}

    run = lambda t: _D().sample_points(x.grid, [t.density, t.vel, t.fuel], t.xyz, [t.out_density, t.out_vel, t.out_fuel])
    return Call({"density": x.f["density"], "vel": x.f["vel"], "fuel": x.f["fuel"], "xyz": x.xyz}, {"out_density": ((n,), F), "out_vel": ((n, 3), F), "out_fuel": ((n,), F)}, run, expect)


def k_trace_points(x):
    def expect(h):
        from points_cases import trace_mirror

        path, status = trace_mirror(x.oracle, h.vel, h.xyz, x.dt, x.inv_dx, 4, 3)
        return {"xyz": path[-1], "status": status}

    run = lambda t: _D().trace_points(x.grid, t.vel, t.xyz, x.dt, x.inv_dx, order=4, steps=3, status=t.status)
    return Call({"vel": x.f["vel"], "xyz": x.xyz}, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("xyz",))


# the collision trace of both levels: PUSH at order 4 with 3 steps and 2 iterations on the harness's 1,031 points, with a threshold above the 0.05 band planted in Ctx.sdf, so
# that hundreds of the points are pushed, put back or left alone (counted on the mirror, never on the library under test)
COLLIDE_THRESHOLD = 0.06
COLLIDE_SPEC = dict(threshold=COLLIDE_THRESHOLD, skin=0.0625, iterations=2)
COLLIDE_ORDER, COLLIDE_STEPS, COLLIDE_MODE = 4, 3, "push"
COLLIDE_VARIANT = "push_order4_steps3"


def _collide_mirror(x, vel, sdf, xyz):
    from points_collide_cases import collide_mirror

    got, status, hit, _ = collide_mirror(x.oracle, vel, sdf, xyz, x.dt, x.inv_dx, COLLIDE_ORDER, COLLIDE_STEPS, COLLIDE_MODE, **COLLIDE_SPEC)
    assert ((hit & 1) != 0).sum() >= 100 and ((hit & 2) != 0).sum() >= 50 and (hit == 0).sum() >= 100, "the case's points meet too little of the collider"
    return got, status, hit


def k_trace_points_collide(x):
    def expect(h):
        got, status, hit = _collide_mirror(x, h.vel, h.sdf, h.xyz)
        return {"xyz": got, "status": status, "hit": hit}

    run = lambda t: _D().trace_points_collide(x.grid, t.vel, t.sdf, t.xyz, x.dt, x.inv_dx, order=COLLIDE_ORDER, steps=COLLIDE_STEPS, mode=COLLIDE_MODE, status=t.status, hit=t.hit,
                                              **COLLIDE_SPEC)
    return Call({"vel": x.f["vel"], "sdf": x.sdf, "xyz": x.xyz}, {"status": ((N_POINTS,), np.uint8), "hit": ((N_POINTS,), np.uint8)}, run, expect, inplace=("xyz",))


def k_splat_points(x):
    """into a float and a Vec3f field at once; the host mirror hns_grid_splat_points gives the expected bytes"""
    def run(t):
        _D().splat_points(x.grid, [t.density, t.vel], t.xyz, [t.vals, t.vals3], status=t.status, rejected=t.rejected)

    def expect(h):
        from hnanosolver_amd import api

        fields, status = [np.array(h.density), np.array(h.vel)], np.zeros(N_POINTS, np.uint8)
        rejected = api.splat_points_host(x.grid, fields, h.xyz, [h.vals, h.vals3], status=status)
        return {"density": fields[0], "vel": fields[1], "status": status, "rejected": np.array([rejected], dtype=np.int64)}

    ins = {"density": x.f["density"], "vel": x.f["vel"], "xyz": x.xyz, "vals": x.values, "vals3": x.values3, "rejected": np.zeros(1, np.int64)}
    return Call(ins, {"status": ((N_POINTS,), np.uint8)}, run, expect, inplace=("density", "vel", "rejected"), poison={"rejected": np.full(1, 12345, np.int64)})


def k_point_leaves(x):
    """synchronous: host results. The positions arrive late; origins, masks and the skipped count against the host mirror"""
    box = {}

    def run(t):
        import torch

        o, m, skipped = _D().point_leaves(t.xyz)
        box["host"] = (o, m, skipped)
        return {"origins": torch.from_numpy(o.reshape(-1)), "masks": torch.from_numpy(m.reshape(-1)), "skipped": torch.tensor([skipped])}

    def expect(h):
        from hnanosolver_amd import leafio

        o, m, skipped = leafio.point_leaves(h.xyz)
        return {"origins": o.reshape(-1), "masks": m.reshape(-1), "skipped": np.array([skipped])}

    return Call({"xyz": x.xyz}, {}, run, expect, asynchronous=False)


def k_field_stats(x):
    def expect(h):
        from hnanosolver_amd import leafio

        return {"rec1": leafio.leaf_stats(h.density, h.masks), "rec3": leafio.leaf_stats(h.vel, None)}

    def run(t):
        _D().field_stats(x.grid, t.density, t.masks, t.rec1)
        _D().field_stats(x.grid, t.vel, None, t.rec3)

    return Call({"density": x.f["density"], "vel": x.f["vel"], "masks": x.masks.reshape(-1)}, {"rec1": ((48,), np.uint8), "rec3": ((144,), np.uint8)}, run, expect,
                poison={"masks": np.ascontiguousarray(~x.masks.reshape(-1))})  # complemented masks: valid, different


def k_residual(x):
    def expect(h):
        from diag_cases import residual_numpy
        from hnanosolver_amd import leafio

        c = residual_numpy(x.origins, h.div, h.p, F(x.vs))
        return {"c": c, "rec": leafio.leaf_stats(c, None)}

    return Call({"div": x.div, "p": x.p_small}, {"c": _flt(x), "rec": ((48,), np.uint8)}, lambda t: _D().residual(x.grid, t.div, t.p, x.vs, t.c, t.rec), expect)


def k_chain(which, iterations=6):
    """advect_vector -> divergence -> rbgs_iterate -> subtract_pressure_gradient on caller tensors: what two streams run side by side on one grid, and what is in
    flight when its grid goes back to the pool (no CASES entry: every call in it has its own)"""
    def build(x):
        D = _D()

        def run(t):
            D.advect_vector(x.grid, t.vel, t.adv, x.dt, x.inv_dx)
            D.divergence(x.grid, t.adv, t.div, x.inv_dx)
            p = D.rbgs_iterate(x.grid, t.div, t.p_a, t.p_b, x.vs, x.omega, iterations)
            D.subtract_pressure_gradient(x.grid, t.adv, p, t.out, x.inv_dx)

        vel = (x.far if which == "far" else x.f)["vel"]
        return Call({"vel": vel, "p_a": np.zeros(x.N, F), "p_b": np.zeros(x.N, F)}, {"adv": _vec(x), "div": _flt(x), "out": _vec(x)}, run, inplace=("p_a", "p_b"))
    return build


# ---------------------------------------------------------------------------------------------------------------------
# sim-level cases: hns_sim_* on a device-resident sim whose state goes up with hns_sim_upload from pinned memory on the late stream
# ---------------------------------------------------------------------------------------------------------------------


class SimCall:
    """run(sim, st, t) after the upload, all on stream st (0: the null stream); t = the late device inputs (points). May return {name: tensor or array}.
    pressure: the pressure of the last solve is part of the result. expect(x, result): further checks against a host mirror."""

    def __init__(self, run, inputs=None, inplace=(), poison=None, asynchronous=True, options=None, pressure=False, expect=None, names=SIM_NAMES):
        self.run, self.inputs, self.inplace, self.poison = run, inputs or (lambda x: {}), tuple(inplace), poison or (lambda x: {})
        self.asynchronous, self.options, self.pressure, self.expect, self.names = asynchronous, options or {}, pressure, expect, names


def params():
    from hnanosolver_amd import api

    return api.CombustionParams(factorScale=1.0)


def nan_state(x, names):
    st = {"vel": np.full((x.N, 3), NAN_WORD, dtype=np.uint32).view(F)}
    for n in names:
        st[n] = np.full(x.N, NAN_WORD, dtype=np.uint32).view(F)
    return st


def collect_sim(sim, names, pressure, extra):
    """everything a sim case compares, on the idle device: fields on the sim's current grid, active masks, look-ahead counts, what run returned"""
    import torch
    from diag_cases import pressure_of
    from frame_cases import download

    torch.cuda.synchronize()
    out = {f"field {k}": v for k, v in download(sim, names).items()}
    out["leaf origins"] = sim.grid.coords()[::512].copy()
    out["masks"] = sim.active_masks()
    if pressure:
        out["pressure"] = pressure_of(sim)
    for k, v in (extra or {}).items():
        out[k] = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return out


def run_sim_case(torch, x, sc, delay, what, late=True, delay_ms=None, stream=None):
    """-> ({name: array}, host seconds, Late or None). late=False: the same calls on the null stream with the device idle before and after."""
    D = _D()
    sim = D.Sim(x.grid, sc.names)
    try:
        sim.upload(nan_state(x, sc.names))  # whatever the late upload does not bring is NaN
        torch.cuda.synchronize()
        state = {k: v for k, v in x.pinned_state().items() if k == "vel" or k in sc.names}
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases' arrays are read-only)
        ins, poison = sc.inputs(x), sc.poison(x)
        staging = {k: dev(v) for k, v in ins.items()}
        t = NS({k: torch.empty_like(v) for k, v in staging.items()})
        operands = {k: Operand(t[k], staging[k], dev(poison[k]) if k in poison else None) for k in ins}

        def fn(stream):
            sim.upload(state, stream)
            return sc.run(sim, stream, t)

        if not late:
            for op in operands.values():
                op.arrive()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = fn(0)
            host = time.perf_counter() - t0
            torch.cuda.synchronize()
            rec = None
            extra = dict(extra or {}, **{k: t[k] for k in sc.inplace})
        else:
            rec = late_call(fn, operands, {k: t[k] for k in sc.inplace}, delay, delay_ms, sc.asynchronous, stream, what)
            host = None
            extra = dict({k: v for k, v in (rec.returned or {}).items() if not torch.is_tensor(v)}, **rec.outputs)
            assert_inputs_unchanged(rec.inputs, ins, sc.inplace, what)
        return collect_sim(sim, sc.names, sc.pressure, extra), host, rec
    finally:
        torch.cuda.synchronize()
        sim.close()


def check_sim_case(torch, x, sc, delay, what):
    import hnanosolver_amd as H

    try:
        for k, v in sc.options.items():
            H.set_option(k, v)
        want, host, _ = run_sim_case(torch, x, sc, delay, what, late=False)
        if sc.expect is not None:
            sc.expect(x, want)
        got, _, rec = run_sim_case(torch, x, sc, delay, what, late=True, delay_ms=delay.for_host_time(host))
        HOST_TIMES[what] = (host, rec.delay_ms)
        assert_same_outputs(got, want, f"{what}, late on a non-blocking stream")
        return got, want
    finally:
        for k in sc.options:
            H.set_option(k, None)


def _points(x):
    return {"xyz": x.xyz}


def s_upload(x):
    return SimCall(lambda sim, st, t: None)


def s_download(x):
    def run(sim, st, t):
        out = {"vel": np.empty((x.N, 3), F), **{k: np.empty(x.N, F) for k in SIM_NAMES}}
        sim.download(out, st)
        return {f"downloaded {k}": v for k, v in out.items()}

    def expect(x, r):
        for k, v in x.state.items():
            assert same_words(r[f"downloaded {k}"], v), k

    return SimCall(run, asynchronous=False, expect=expect)


def s_substep(coll):
    return lambda x: SimCall(lambda sim, st, t: sim.substep(9, x.dt, x.vs, params(), coll, st), pressure=True)


def s_core_substep(x):
    def run(sim, st, t):
        sim.core_substep(7, x.dt, x.vs, st)
        sim.core_substep(7, x.dt, x.vs, st)  # (the second finds the first's look-ahead under lookahead = auto's rule or not: either way the same bytes)

    return SimCall(run, pressure=True)


def s_advect(x):
    return SimCall(lambda sim, st, t: sim.advect(None, True, dt=x.dt, voxel_size=x.vs, stream=st))


def s_pressure_solve(options, iterations=7):
    """behind a core substep on the same stream, which leaves the pressure buffers dirty: the solve's start from zero must come after it"""
    def build(x):
        def run(sim, st, t):
            sim.core_substep(4, x.dt, x.vs, st)
            sim.pressure_solve(iterations, x.vs, st)

        return SimCall(run, pressure=True, options=options)
    return build


def s_pressure_solve_controlled(x):
    """with a solve control the host waits once per check: synchronous in effect"""
    def run(sim, st, t):
        sim.core_substep(4, x.dt, x.vs, st)
        sim.solve_control(rel_tol=1e-3, check_every=4)
        sim.pressure_solve(40, x.vs, st)
        r = sim.solve_report()
        return {"iterations": np.array([r["iterations"], r["checks"], int(r["converged"])]), "history": r["history"]}

    return SimCall(run, pressure=True, asynchronous=False)


def s_sample(x):
    def expect(x, r):
        from points_cases import fma_branch

        for k in SIM_NAMES:
            assert same_words(r[f"sampled {k}"], x.oracle.sample_trilinear_f(x.state[k], x.xyz)), f"hns_sim_sample_points on the null stream differs from the oracle in {k}"
        with fma_branch(x.oracle.L):
            assert same_words(r["sampled vel"], x.oracle.sample_trilinear_v(x.state["vel"], x.xyz)), "hns_sim_sample_points on the null stream differs from the oracle in vel"

    return SimCall(lambda sim, st, t: {f"sampled {k}": v for k, v in sim.sample(None, t.xyz, velocity=True, stream=st).items()}, _points, expect=expect)


def s_trace(x):
    def expect(x, r):
        from points_cases import trace_mirror

        path, status = trace_mirror(x.oracle, x.state["vel"], x.xyz, x.dt, x.inv_dx, 4, 3)
        assert same_words(r["xyz"], path[-1]) and same_words(r["status"], status), "hns_sim_trace_points on the null stream differs from points_cases.trace_mirror"

    return SimCall(lambda sim, st, t: {"status": sim.trace(t.xyz, dt=x.dt, voxel_size=x.vs, order=4, steps=3, status=True, stream=st)}, _points, inplace=("xyz",), expect=expect)


def s_trace_collide(x):
    def expect(x, r):
        got, status, hit = _collide_mirror(x, x.state["vel"], x.state["collision_sdf"], x.xyz)
        assert same_words(r["xyz"], got) and same_words(r["status"], status) and same_words(r["hit"], hit), \
            "hns_sim_trace_points_collide on the null stream differs from points_collide_cases.collide_mirror"

    def run(sim, st, t):
        status, hit = sim.trace(t.xyz, dt=x.dt, voxel_size=x.vs, order=COLLIDE_ORDER, steps=COLLIDE_STEPS, status=True, stream=st, collide=COLLIDE_MODE, hit=True, **COLLIDE_SPEC)
        return {"status": status, "hit": hit}

    return SimCall(run, _points, inplace=("xyz",), expect=expect)


def s_splat(x):
    def run(sim, st, t):
        sim.set_active_masks(x.masks, st)
        return {"status": sim.splat({"density": t.vals, "fuel": t.vals}, t.xyz, velocity=t.vals3, status=True, rejected=t.rejected, stream=st)}

    def expect(x, r):
        from hnanosolver_amd import api

        fields, masks = [np.array(x.state["density"]), np.array(x.state["fuel"]), np.array(x.state["vel"])], np.array(x.masks)
        status = np.zeros(N_POINTS, np.uint8)
        rejected = api.splat_points_host(x.grid, fields, x.xyz, [x.values, x.values, x.values3], masks=masks, status=status)
        for k, v in {"field density": fields[0], "field fuel": fields[1], "field vel": fields[2], "masks": masks, "status": status, "rejected": np.array([rejected])}.items():
            assert same_words(r[k], v), f"hns_sim_splat_points on the null stream differs from the host mirror in {k}"

    ins = lambda x: {"xyz": x.xyz, "vals": x.values, "vals3": x.values3, "rejected": np.zeros(1, np.int64)}
    return SimCall(run, ins, inplace=("rejected",), expect=expect)


def s_set_masks(x):
    def expect(x, r):
        assert same_words(r["masks"], x.masks)

    return SimCall(lambda sim, st, t: sim.set_active_masks(x.masks, st), expect=expect)


def s_get_masks(x):
    def run(sim, st, t):
        sim.set_active_masks(x.masks, st)
        return {"read back": sim.active_masks(st)}

    def expect(x, r):
        assert same_words(r["read back"], x.masks)

    return SimCall(run, asynchronous=False, expect=expect)


TOLERANCES = {"density": 0.3, "temperature": 30.0}


def _deactivate_expect(x, r):
    from hnanosolver_amd import leafio

    m, counts = leafio.deactivate_masks(x.masks, {k: (x.state[k], tol) for k, tol in TOLERANCES.items()}, (x.state["vel"], 1.0))
    assert same_words(r["masks"], m), "hns_sim_deactivate on the null stream differs from the host mirror"
    if "counts" in r:
        assert tuple(r["counts"]) == counts


def s_deactivate(counts):
    def build(x):
        def run(sim, st, t):
            sim.set_active_masks(x.masks, st)
            c = sim.deactivate(TOLERANCES, velocity=1.0, counts=counts, stream=st)
            return {"counts": np.array(c)} if counts else None

        return SimCall(run, asynchronous=not counts, expect=_deactivate_expect)
    return build


def s_stats(x):
    def run(sim, st, t):
        sim.set_active_masks(x.masks, st)
        return {"masked": sim.stats(["density", "flame"], velocity=True, masks=True, stream=st), "all": sim.stats(["fuel"], masks=False, stream=st)}

    def expect(x, r):
        from hnanosolver_amd import leafio

        want = np.concatenate([leafio.leaf_stats(x.state[k], x.masks) for k in ("density", "flame", "vel")])
        assert same_words(r["masked"], want) and same_words(r["all"], leafio.leaf_stats(x.state["fuel"], None)), "hns_sim_stats differs from the host mirror"

    return SimCall(run, asynchronous=False, expect=expect)


def s_residual(x):
    def run(sim, st, t):
        sim.core_substep(7, x.dt, x.vs, st)
        return {"record": sim.residual(x.vs, st)}

    return SimCall(run, asynchronous=False, pressure=True)


def s_regrid(kind):
    """the regrid, a download of what it made, then a substep on the new grid, all on the late stream; domain, masks and fields against the host chain"""
    def build(x):
        from frame_cases import host_chain, make_sources, sdf_source
        from seed_cases import host_chain_seeded

        sdf, sources = sdf_source(4, x.origins), make_sources(6, x.origins, "mixed", "edge")

        def run(sim, st, t):
            sim.set_active_masks(x.masks, st)
            if kind == "plain":
                sim.regrid(1, sdf=sdf, stream=st)
            elif kind == "sourced":
                sim.regrid(2, sources=sources, stream=st)
            else:
                sim.regrid(1, points=t.xyz, stream=st)
            n = sim.grid.voxel_count()
            made = {"vel": np.empty((n, 3), F), **{k: np.empty(n, F) for k in SIM_NAMES}}
            sim.download(made, st)
            sim.substep(5, x.dt, x.vs, params(), False, st)
            return {"seeds skipped": np.array([sim.last_seeds_skipped]), **{f"regridded {k}": v for k, v in made.items()}}

        def expect(x, r):
            if kind == "plain":
                dom, dm, out = host_chain(x.origins, x.masks, x.state, SIM_NAMES, 1, None, sdf)
            elif kind == "sourced":
                dom, dm, out = host_chain(x.origins, x.masks, x.state, SIM_NAMES, 2, sources, None)
            else:
                dom, dm, out = host_chain_seeded(x.origins, x.masks, x.state, SIM_NAMES, 1, x.xyz)
            assert same_words(r["leaf origins"], dom) and same_words(r["masks"], dm), f"regrid ({kind}) on the null stream: domain or masks differ from the host chain"
            for k, v in out.items():
                assert same_words(r[f"regridded {k}"], v), f"regrid ({kind}) on the null stream: field {k} differs from the host chain"

        return SimCall(run, _points if kind == "seeded" else None, asynchronous=False, expect=expect)
    return build


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in operators: host pointers in, results in place, synchronous; the stream they are given is busy with the delay
# ---------------------------------------------------------------------------------------------------------------------


def operator_run(x, name, stream, feedback=False):
    """one operator on fresh data of grid x, on a handle whose cook cache holds another cook's state -> {block: array}"""
    from hnanosolver_amd import api
    from operator_cases import build_data, snapshot

    coll = name == "hns_compute_sim"  # the plain cook with a collision field, the feedback cooks without
    d = build_data(x.origins, x.R, with_sdf=coll, amplitude=400.0 if "advect" in name else 160.0)
    if name == "hns_divergence":
        d.addValueBlock("divergence", d.FLOAT)
    h = api.IndexGridHandle()
    api.CreateIndexGrid(d, h, x.vs)
    try:
        if name in ("hns_compute_sim", "hns_compute_sim_resident"):
            stale = build_data(x.origins, x.R, with_sdf=coll, amplitude=96.0)
            api.Compute_Sim(stale, h, 3, x.dt, x.vs, params(), coll)  # the cache now holds state that is not this cook's
            import torch

            torch.cuda.synchronize()
            out = {}
            with_delay = stream["enqueue"]
            with_delay()
            api.Compute_Sim(d, h, 9, x.dt, x.vs, params(), coll, stream=stream["handle"])
            out.update({f"cook 1 {k}": v for k, v in snapshot(d).items()})
            if name == "hns_compute_sim_resident":
                for checked in (False, True):
                    with_delay()
                    skipped = api.Compute_Sim(d, h, 9, x.dt, x.vs, params(), coll, stream=stream["handle"], feedback=True, checked=checked)
                    out.update({f"feedback cook checked={checked} {k}": v for k, v in snapshot(d).items()})
                    out[f"uploads skipped checked={checked}"] = np.array([skipped])
            return out
        stream["enqueue"]()
        op = {"hns_advect_index_grid": lambda: api.AdvectIndexGrid(d, x.dt, x.vs, stream=stream["handle"], handle=h),
              "hns_advect_index_grid_velocity": lambda: api.AdvectIndexGridVelocity(d, x.dt, x.vs, stream=stream["handle"], handle=h),
              "hns_project_non_divergent": lambda: api.ProjectNonDivergent(d, 7, x.vs, stream=stream["handle"], handle=h),
              "hns_divergence": lambda: api.Divergence(d, x.vs, stream=stream["handle"], handle=h)}[name]
        op()
        return snapshot(d)
    finally:
        h.reset()


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------

Entry = namedtuple("Entry", "level source grids variants")  # variants: {id: builder(x)}
BOTH, SCATTERED, PLUME = ("scattered", "plume"), ("scattered",), ("plume",)
ORACLE = "oracle (OracleGrid) and the null stream"
MIRROR = "host mirror and the null stream"
NULL = "the same call on the null stream, device idle before and after"

_SOR = {f"{o}_x{n}": k_rbgs_iterate(opts, n) for o, opts in (("leaf_blocks", {"sor_block_lb": "1"}), ("16cube_blocks", {"sor_block_lb": "2"}), ("color", {"rbgs": "color"}))
        for n in (4, 2, 7)}  # 4 / 2 / 1 iterations per launch all occur: 7 = 4 + 2 + 1 on small one-leaf blocks, 2 + 2 + 2 + 1 elsewhere

CASES = {
    # kernel level (hns_dev_*): late_call with the outputs carved from a Slab
    "hns_dev_advect_vector": Entry("kernel", ORACLE, BOTH, {"plain": k_advect_vector(False), "collision": k_advect_vector(True)}),
    "hns_dev_advect_scalar": Entry("kernel", ORACLE, BOTH, {"plain": k_advect_scalar(False), "collision": k_advect_scalar(True)}),
    "hns_dev_advect_scalars": Entry("kernel", ORACLE, BOTH, {"plain": k_advect_scalars(False), "collision": k_advect_scalars(True)}),
    "hns_dev_advect_scalar_multi": Entry("kernel", ORACLE, BOTH, {"plain": k_advect_scalar_multi(False), "collision": k_advect_scalar_multi(True)}),
    "hns_dev_advect_scalars_ahead": Entry("kernel", ORACLE, BOTH, {"plain": k_advect_scalars_ahead}),
    "hns_dev_divergence": Entry("kernel", ORACLE, BOTH, {"plain": k_divergence}),
    "hns_dev_rbgs_color": Entry("kernel", ORACLE, BOTH, {"red_black_red": k_rbgs_color}),
    "hns_dev_rbgs_iterate": Entry("kernel", ORACLE, BOTH, _SOR),
    "hns_dev_subtract_pressure_gradient": Entry("kernel", ORACLE, BOTH, {"plain": k_gradient(False), "collision": k_gradient(True)}),
    "hns_dev_combustion_oxygen": Entry("kernel", ORACLE, SCATTERED, {"plain": k_combustion}),
    "hns_dev_temperature_buoyancy": Entry("kernel", ORACLE, SCATTERED, {"plain": k_buoyancy}),
    "hns_dev_vorticity_confinement": Entry("kernel", ORACLE, BOTH, {"factor_scale_1": k_vorticity(1.0), "factor_scale_2": k_vorticity(2.0)}),
    "hns_dev_enforce_collision_boundaries": Entry("kernel", ORACLE, BOTH, {"plain": k_enforce}),
    "hns_dev_pack_leaves": Entry("kernel", "numpy indexing and the null stream", SCATTERED, {"float": k_pack(1), "vec3": k_pack(3)}),
    "hns_dev_unpack_leaves": Entry("kernel", "numpy indexing and the null stream", SCATTERED, {"float": k_unpack(1), "vec3": k_unpack(3)}),
    "hns_dev_sample_points": Entry("kernel", ORACLE + " (sample_trilinear_f / _v)", SCATTERED, {"float_vec3_float": k_sample_points}),
    "hns_dev_trace_points": Entry("kernel", MIRROR + " (points_cases.trace_mirror)", SCATTERED, {"order4_steps3": k_trace_points}),
    "hns_dev_trace_points_collide": Entry("kernel", MIRROR + " (points_collide_cases.collide_mirror)", SCATTERED, {COLLIDE_VARIANT: k_trace_points_collide}),
    "hns_dev_splat_points": Entry("kernel", MIRROR + " (hns_grid_splat_points)", SCATTERED, {"float_and_vec3": k_splat_points}),
    "hns_dev_point_leaves": Entry("kernel", MIRROR + " (hns_point_leaves)", SCATTERED, {"plain": k_point_leaves}),
    "hns_dev_field_stats": Entry("kernel", MIRROR + " (hns_leaf_stats)", BOTH, {"masked_float_and_vec3": k_field_stats}),
    "hns_dev_residual": Entry("kernel", MIRROR + " (diag_cases.residual_numpy, hns_leaf_stats)", BOTH, {"plain": k_residual}),
    # sim level (hns_sim_*): the state goes up with hns_sim_upload from pinned memory on the late stream, then the call(s)
    "hns_sim_upload": Entry("sim", NULL, SCATTERED, {"plain": s_upload}),
    "hns_sim_download": Entry("sim", "the uploaded arrays and the null stream", SCATTERED, {"plain": s_download}),
    "hns_sim_substep": Entry("sim", NULL, BOTH, {"plain": s_substep(False), "collision": s_substep(True)}),
    "hns_sim_core_substep": Entry("sim", NULL, BOTH, {"two": s_core_substep}),
    "hns_sim_advect": Entry("sim", NULL, SCATTERED, {"all_fields_and_velocity": s_advect}),
    "hns_sim_pressure_solve": Entry("sim", NULL, BOTH, {"plain": s_pressure_solve({}), "color": s_pressure_solve({"rbgs": "color"}),
                                                        "solve_control": s_pressure_solve_controlled}),
    "hns_sim_sample_points": Entry("sim", ORACLE + " (sample_trilinear_f / _v)", SCATTERED, {"all_fields_and_velocity": s_sample}),
    "hns_sim_trace_points": Entry("sim", MIRROR + " (points_cases.trace_mirror)", SCATTERED, {"order4_steps3": s_trace}),
    "hns_sim_trace_points_collide": Entry("sim", MIRROR + " (points_collide_cases.collide_mirror)", SCATTERED, {COLLIDE_VARIANT: s_trace_collide}),
    "hns_sim_splat_points": Entry("sim", MIRROR + " (hns_grid_splat_points)", SCATTERED, {"two_floats_and_velocity": s_splat}),
    "hns_sim_set_active_masks": Entry("sim", "the masks set and the null stream", SCATTERED, {"plain": s_set_masks}),
    "hns_sim_active_masks": Entry("sim", "the masks set and the null stream", SCATTERED, {"plain": s_get_masks}),
    "hns_sim_deactivate": Entry("sim", MIRROR + " (hns_deactivate_leaf_masks)", SCATTERED, {"asynchronous": s_deactivate(False), "counts": s_deactivate(True)}),
    "hns_sim_stats": Entry("sim", MIRROR + " (hns_leaf_stats)", SCATTERED, {"plain": s_stats}),
    "hns_sim_residual": Entry("sim", NULL, SCATTERED, {"plain": s_residual}),
    "hns_sim_regrid": Entry("sim", MIRROR + " (frame_cases.host_chain)", SCATTERED, {"sdf_source_then_substep": s_regrid("plain")}),
    "hns_sim_regrid_sourced": Entry("sim", MIRROR + " (frame_cases.host_chain)", SCATTERED, {"mixed_sources_then_substep": s_regrid("sourced")}),
    "hns_sim_regrid_seeded": Entry("sim", MIRROR + " (seed_cases.host_chain_seeded)", SCATTERED, {"points_then_substep": s_regrid("seeded")}),
    # the operators (host pointers): synchronous, on a stream that is busy with the delay, cook_pipeline on and off
    "hns_compute_sim": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
    "hns_compute_sim_resident": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
    "hns_advect_index_grid": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
    "hns_advect_index_grid_velocity": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
    "hns_project_non_divergent": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
    "hns_divergence": Entry("operator", NULL, PLUME, {"pipeline_1": "1", "pipeline_0": "0"}),
}

_DIST = "run on the ranks' own compute and communication streams by tests/test_dist_gpu.py"
EXEMPT = {
    "hns_dist_upload": _DIST,
    "hns_dist_download": _DIST,
    "hns_dist_download_local": _DIST,
    "hns_dist_core_substep": _DIST,
    "hns_dist_local_core_substep": _DIST,
    "hns_dist_sim_substep": _DIST,
    "hns_dist_local_sim_substep": _DIST,
    "hns_dist_synchronize": _DIST,
    "hns_dev_time_rbgs": "a timing helper around hns_dev_rbgs_iterate, which is a case; it waits for its own events and returns no field",
}


def variants(level):
    """[(entry point, variant id, grid name)] of one level, for pytest.mark.parametrize"""
    return [(name, v, g) for name, e in CASES.items() if e.level == level for v in e.variants for g in e.grids]


def stream_entry_points(header_text):
    """the functions include/hns.h declares with a `void* stream` parameter"""
    import re

    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(hns_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out
