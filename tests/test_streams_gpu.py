"""The stream contract of include/hns.h, held on the GPU: every call that takes a `void* stream` is ordered on THAT stream and on nothing else, and writes its
outputs and nothing else.

Each case of tests/stream_cases.py runs once on the null stream with the device idle (where its host time is taken and its bytes are compared with the oracle or a
host mirror) and once LATE: on a non-blocking stream on which the true inputs arrive behind a delay of at least ten times that host time, everything holding poison
until then, outputs carved from a guard-banded slab. The late bytes must equal the null-stream bytes, the guards must be intact and the inputs unchanged; an asynchronous
call must have returned while the delay was still running (`armed`), or the case fails as having tested nothing. Then the compositions: the lazy block-record build on
a late stream, the look-ahead memo across two streams, two streams on one grid, pooled memory changing owner with work in flight -- and one planted ordering bug, which
the harness must see.

Delays: every CASES entry gets ten times its own measured host time (2 ms at the least). The compositions use fixed delays of 2 - 20 ms, one to two orders above the
host time of what they enqueue; (c), (d), (e) and (f) assert `armed`. The operator cases and (b) are synchronous calls: the stream they are given is busy when they
are called, but nothing can show that it still was when their device work was enqueued.

Host times and delays measured on an MI355X: stream_cases.HOST_TIMES, printed by test_report at the end of this module.
"""
import numpy as np
import pytest

import hnanosolver_amd as H
import stream_cases as sc

pytestmark = pytest.mark.gpu

OPTIONS = ("rbgs", "sor_block_lb", "cook_pipeline", "lookahead")
_CTX = {}


def ctx(name):
    if name not in _CTX:
        _CTX[name] = sc.Ctx(name)
    return _CTX[name]


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def delay(torch):
    return sc.Delay(torch)


@pytest.fixture(autouse=True)
def default_options():
    yield
    for k in OPTIONS:
        H.set_option(k, None)


def ids(v):
    return [f"{n}-{variant}-{grid}" for n, variant, grid in v]


# ---------------------------------------------------------------------------------------------------------------
# (a) every case, late
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,variant,grid", sc.variants("kernel"), ids=ids(sc.variants("kernel")))
def test_kernel_level_call_late_and_guard_banded(name, variant, grid, torch, delay):
    x = ctx(grid)
    sc.check_call(torch, sc.CASES[name].variants[variant](x), delay, f"{name}[{variant}-{grid}]")


@pytest.mark.parametrize("name,variant,grid", sc.variants("sim"), ids=ids(sc.variants("sim")))
def test_sim_level_call_late(name, variant, grid, torch, delay):
    x = ctx(grid)
    sc.check_sim_case(torch, x, sc.CASES[name].variants[variant](x), delay, f"{name}[{variant}-{grid}]")


@pytest.mark.parametrize("name,variant,grid", sc.variants("operator"), ids=ids(sc.variants("operator")))
def test_operator_on_a_busy_non_blocking_stream(name, variant, grid, torch, delay):
    """synchronous calls: no `armed`. The pipelined cook must hand its work between the caller's stream -- busy with the delay -- and its transfer stream in order"""
    x = ctx(grid)
    H.set_option("cook_pipeline", sc.CASES[name].variants[variant])
    torch.cuda.synchronize()
    want = sc.operator_run(x, name, {"handle": None, "enqueue": lambda: None})
    torch.cuda.synchronize()
    S = torch.cuda.Stream()

    def enqueue():
        with torch.cuda.stream(S):
            delay.enqueue(5.0)

    got = sc.operator_run(x, name, {"handle": S, "enqueue": enqueue})
    torch.cuda.synchronize()
    sc.assert_same_outputs(got, want, f"{name}[{variant}] on a busy non-blocking stream")


# ---------------------------------------------------------------------------------------------------------------
# (b) first use on a late stream: the lazy block-record build
# ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("grid", ["scattered", "plume"])
def test_first_launch_on_a_grid_is_on_a_late_stream(grid, torch, delay):
    """hns_grid_build_blocks runs inside the first rbgs_iterate with 16^3 blocks, on a private stream it waits for: results only, no `armed`"""
    x = ctx(grid).with_fresh_grid()
    assert x.grid.ptr  # made here (making a grid waits for the device) and never launched on
    call = sc.k_rbgs_iterate({"sor_block_lb": "2"}, 4)(x)
    H.set_option("sor_block_lb", "2")
    b = sc.Bench(torch, call)
    late = b.late(delay, 5.0, f"first rbgs_iterate on {grid}", asynchronous=False)
    b.slab.check("first use, late")
    want = call.expect(sc.NS(call.inputs))["result"]
    assert sc.same_words(late.outputs["result"], want), "the first rbgs_iterate on a grid, late on a non-blocking stream, differs from the oracle"
    ref, _, _ = b.on_null_stream()  # (the records exist now)
    sc.assert_same_outputs(late.outputs, ref, "first use late against the second use on the null stream")
    sc.assert_inputs_unchanged(late.inputs, call.inputs, call.inplace, "first use, late")


# ---------------------------------------------------------------------------------------------------------------
# (c) the look-ahead memo from one stream to the next
# ---------------------------------------------------------------------------------------------------------------


def test_lookahead_memo_crosses_streams(torch, delay):
    """core_substep on S1 behind a delay leaves advect_vector of the next substep in the sim; S2 waits for S1 and runs that substep, which skips its own launch.
    Counts: (1, 0) after the first call. The second consumes the one memo there is -- and, under lookahead = 1, looks ahead itself: (2, 1) in the end."""
    from frame_cases import download
    from hnanosolver_amd import device as D

    x = ctx("scattered")
    names = [n for n in sc.SIM_NAMES if n != "collision_sdf"]
    state = {k: v for k, v in x.pinned_state().items() if k == "vel" or k in names}

    def two_substeps(mode, streams):
        H.set_option("lookahead", mode)
        sim = D.Sim(x.grid, names)
        try:
            sim.upload(state)
            torch.cuda.synchronize()
            if streams is None:
                sim.core_substep(7, x.dt, x.vs, 0)
                sim.core_substep(7, x.dt, x.vs, 0)
                held, counts = True, None
            else:
                S1, S2 = streams
                armed = torch.cuda.Event()
                with torch.cuda.stream(S1):
                    delay.enqueue(5.0)
                    armed.record(S1)
                sim.core_substep(7, x.dt, x.vs, int(S1.cuda_stream))
                first = sim.lookahead_counts()
                S2.wait_stream(S1)
                sim.core_substep(7, x.dt, x.vs, int(S2.cuda_stream))
                held, counts = not armed.query(), (first, sim.lookahead_counts())
                S2.synchronize()
                S1.synchronize()
            torch.cuda.synchronize()
            return download(sim, names), held, counts
        finally:
            torch.cuda.synchronize()
            sim.close()

    want, _, _ = two_substeps("0", None)
    got, held, counts = two_substeps("1", (torch.cuda.Stream(), torch.cuda.Stream()))
    assert held, "the delay had drained when the second substep was enqueued: the case tested nothing"
    assert counts[0] == (1, 0), counts
    assert counts[1][1] == 1 and counts[1][0] == 2, counts
    sc.assert_same_outputs(got, want, "two core substeps, S1 then S2, against two on the null stream")


# ---------------------------------------------------------------------------------------------------------------
# (d) two streams, one grid
# ---------------------------------------------------------------------------------------------------------------


def test_two_streams_share_one_grid(torch, delay):
    """advect_vector + divergence + rbgs_iterate + subtract_pressure_gradient on S1 and on S2 at once, same grid handle, different fields (no splat: include/hns.h wants the
    calls of one grid's accumulator on one stream)"""
    x = ctx("scattered")
    benches = [sc.Bench(torch, sc.k_chain(which)(x)) for which in ("far", "near")]
    want = [b.on_null_stream() for b in benches]
    ms = delay.for_host_time(max(w[2] for w in want))
    runs = [b.late_run(delay, ms) for b in benches]
    for r in runs:
        r.prepare()
    for r in runs:
        r.launch()
    got = [r.finish(True, f"chain {i} of two on one grid") for i, r in enumerate(runs)]
    assert not sc.same_words(want[0][0]["out"], want[1][0]["out"])
    for i, (b, g, w) in enumerate(zip(benches, got, want)):
        sc.assert_same_outputs(g.outputs, w[0], f"chain {i} beside another stream on the same grid")
        b.slab.check(f"chain {i}")
        sc.assert_inputs_unchanged(g.inputs, b.call.inputs, b.call.inplace, f"chain {i}")


# ---------------------------------------------------------------------------------------------------------------
# (e) the pool's promise: memory changes owner with work in flight
# ---------------------------------------------------------------------------------------------------------------


def test_grid_memory_changes_owner_with_a_chain_in_flight(torch, delay):
    """A chain in flight on S1 behind a delay; its grid is destroyed (tables and block records go to the pool, which waits for the device); a grid of ANOTHER topology
    with the same leaf count -- the mirrored lattice -- draws that memory, fills it with its own origins, neighbour table, hash and launch order, and runs the chain on
    S2 with its own inputs: both results right. Were the pool not to wait, chain a would walk the second grid's tables: every index in range, wrong values."""
    x, y = ctx("scattered"), ctx("mirrored")
    assert y.nl == x.nl and not sc.same_words(x.origins, y.origins)
    want = [sc.Bench(torch, sc.k_chain("far")(x)).on_null_stream()[0], sc.Bench(torch, sc.k_chain("near")(y)).on_null_stream()[0]]
    H.load_library().hns_trim_memory()
    xa, yb = x.with_fresh_grid(), y.with_fresh_grid()
    assert xa.grid.ptr and xa.grid.ptr != x.grid.ptr  # (made here: making a grid waits for the device)
    ba = sc.Bench(torch, sc.k_chain("far")(xa))
    ra = ba.late_run(delay, 20.0).prepare().launch()
    assert ra.held, "the delay had drained when the chain was enqueued"
    xa.grid.reset()  # with the chain in flight
    assert yb.grid.ptr  # made now: it draws what xa's grid gave back and writes its own tables there
    bb = sc.Bench(torch, sc.k_chain("near")(yb))
    rb = bb.late_run(delay, 5.0).prepare().launch()
    got_b = rb.finish(False, "chain on the grid that drew the memory")
    got_a = ra.finish(False, "chain whose grid was destroyed in flight")
    sc.assert_same_outputs(got_a.outputs, want[0], "the chain whose grid was destroyed while it was in flight")
    sc.assert_same_outputs(got_b.outputs, want[1], "the chain on the grid that drew the pooled memory")
    ba.slab.check("chain a")
    bb.slab.check("chain b")


def test_sim_memory_changes_owner_with_a_substep_in_flight(torch, delay):
    """Sim.close() with an upload and a substep in flight on S1, then a new sim of equal size, which draws that memory, with OTHER inputs on S2 behind a shorter delay:
    the new sim's result is the serial one. Were hns_sim_destroy not to wait, the first sim's upload and substep (other fields, another dt and iteration count) would
    land in the second sim's fields after its own work."""
    from frame_cases import download
    from hnanosolver_amd import device as D

    x = ctx("scattered")
    names = sc.SIM_NAMES
    state, other = x.pinned_state(), x.pinned_state("far_state")
    assert not sc.same_words(state["vel"], other["vel"]) and not sc.same_words(state["density"], other["density"])

    def substep(sim, st):
        sim.upload(state, st)
        sim.substep(9, x.dt, x.vs, sc.params(), False, st)

    H.load_library().hns_trim_memory()
    sim = D.Sim(x.grid, names)
    substep(sim, 0)
    torch.cuda.synchronize()
    want = download(sim, names)
    sim.close()
    a = D.Sim(x.grid, names)
    a.upload(sc.nan_state(x, names))
    torch.cuda.synchronize()
    S1, S2, armed = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(S1):
        delay.enqueue(20.0)
        armed.record(S1)
    a.upload(other, int(S1.cuda_stream))
    a.substep(5, 0.5 * x.dt, x.vs, sc.params(), False, int(S1.cuda_stream))
    assert not armed.query(), "the delay had drained when the substep was enqueued"
    a.close()  # in flight: its memory goes to the pool, which waits for the device
    b = D.Sim(x.grid, names)  # draws it
    try:
        with torch.cuda.stream(S2):
            delay.enqueue(2.0)
        substep(b, int(S2.cuda_stream))
        S2.synchronize()
        torch.cuda.synchronize()
        sc.assert_same_outputs(download(b, names), want, "the sim that drew the memory of one closed in flight")
    finally:
        torch.cuda.synchronize()
        b.close()


# ---------------------------------------------------------------------------------------------------------------
# (f) the harness bites
# ---------------------------------------------------------------------------------------------------------------


def test_harness_sees_a_planted_ordering_bug(torch, delay):
    """The bug is the test's own: the true inputs arrive on S1 behind the delay, the call goes to a second non-blocking stream S2 with no event between the two. It reads
    the NaN poison -- valid memory, wrong values, no fault -- and the result must DIFFER from the expected bytes."""
    x = ctx("scattered")
    call = sc.CASES["hns_dev_divergence"].variants["plain"](x)
    b = sc.Bench(torch, call)
    ref, _, _ = b.on_null_stream()
    assert sc.same_words(ref["div"], call.expect(sc.NS(call.inputs))["div"])
    late = b.late_run(delay, 20.0, call_stream=torch.cuda.Stream()).prepare().launch().finish(True, "planted bug")
    assert not sc.same_words(late.outputs["div"], ref["div"]), "a call that was NOT ordered behind its inputs' stream still gave the expected bytes: the harness sees nothing"
    got = late.outputs["div"].cpu().numpy()
    assert np.isnan(got).mean() > 0.9  # it read the poison
    b.slab.check("planted bug")  # (wrong values, but where they belong)


def test_report(torch, delay):
    """prints what the module measured: the host time of every case on the null stream and the delay enqueued in front of its late run"""
    rows = sorted(sc.HOST_TIMES.items())
    print(f"\none delay operation: {delay.ms_per_op * 1e3:.1f} us of GPU time; floor {sc.MIN_DELAY_MS} ms; factor {sc.DELAY_FACTOR}")
    for what, (host, ms) in rows:
        print(f"  {what:78s} host {host * 1e6:9.1f} us   delay {ms:7.2f} ms")
    if rows:
        hosts = np.array([h for h, _ in sc.HOST_TIMES.values()]) * 1e6
        print(f"host time: min {hosts.min():.1f} us, median {np.median(hosts):.1f} us, max {hosts.max():.1f} us over {len(rows)} cases")
        assert all(ms >= sc.DELAY_FACTOR * host * 1e3 and ms >= sc.MIN_DELAY_MS for host, ms in sc.HOST_TIMES.values())
