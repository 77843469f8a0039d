"""TEST HELPER of tests/test_points_collide_gpu.py and tests/test_points_collide_abi.py: the two collision-tracing entry points as cases of the late-stream harness
(tests/stream_cases.py) and as an exemption of the call-sequence vocabulary (tests/sequence_cases.py).

Both tables are asked about every new entry point by the coverage tests that read them (tests/test_stream_cases.py: every call with a `void* stream` parameter is a case
or exempt; tests/test_sequence_cases.py: every hns_sim_* call is an operation or exempt). The entries of this feature live HERE, next to the feature's other tests, and
join the tables when this module is imported -- which the collection of tests/test_points_collide_*.py does, before any test runs. tests/test_streams_gpu.py is
collected after those files, so its parametrised tests run the two cases as well; tests/test_points_collide_gpu.py runs them itself and does not depend on that order.

The cases: PUSH at order 4 with 3 steps and 2 iterations on the harness's 1,031 points, with a threshold above the 0.05 band planted in Ctx.sdf, so that hundreds of the
points are pushed, put back or left alone (counted on the mirror, never on the library under test)."""
import numpy as np

import sequence_cases as sq
import stream_cases as sc

COLLIDE_THRESHOLD = 0.06
SPEC = dict(threshold=COLLIDE_THRESHOLD, skin=0.0625, iterations=2)
ORDER, STEPS, MODE = 4, 3, "push"


def _mirror(x, vel, sdf, xyz):
    from points_collide_cases import collide_mirror

    got, status, hit, _ = collide_mirror(x.oracle, vel, sdf, xyz, x.dt, x.inv_dx, ORDER, STEPS, MODE, **SPEC)
    assert ((hit & 1) != 0).sum() >= 100 and ((hit & 2) != 0).sum() >= 50 and (hit == 0).sum() >= 100, "the case's points meet too little of the collider"
    return got, status, hit


def k_trace_points_collide(x):
    def expect(h):
        got, status, hit = _mirror(x, h.vel, h.sdf, h.xyz)
        return {"xyz": got, "status": status, "hit": hit}

    run = lambda t: sc._D().trace_points_collide(x.grid, t.vel, t.sdf, t.xyz, x.dt, x.inv_dx, order=ORDER, steps=STEPS, mode=MODE, status=t.status, hit=t.hit, **SPEC)
    return sc.Call({"vel": x.f["vel"], "sdf": x.sdf, "xyz": x.xyz}, {"status": ((sc.N_POINTS,), np.uint8), "hit": ((sc.N_POINTS,), np.uint8)}, run, expect, inplace=("xyz",))


def s_trace_collide(x):
    def expect(x, r):
        got, status, hit = _mirror(x, x.state["vel"], x.state["collision_sdf"], x.xyz)
        assert sc.same_words(r["xyz"], got) and sc.same_words(r["status"], status) and sc.same_words(r["hit"], hit), \
            "hns_sim_trace_points_collide on the null stream differs from points_collide_cases.collide_mirror"

    def run(sim, st, t):
        status, hit = sim.trace(t.xyz, dt=x.dt, voxel_size=x.vs, order=ORDER, steps=STEPS, status=True, stream=st, collide=MODE, hit=True, **SPEC)
        return {"status": status, "hit": hit}

    return sc.SimCall(run, sc._points, inplace=("xyz",), expect=expect)


VARIANT = "push_order4_steps3"
CASES = {
    "hns_dev_trace_points_collide": sc.Entry("kernel", sc.MIRROR + " (points_collide_cases.collide_mirror)", sc.SCATTERED, {VARIANT: k_trace_points_collide}),
    "hns_sim_trace_points_collide": sc.Entry("sim", sc.MIRROR + " (points_collide_cases.collide_mirror)", sc.SCATTERED, {VARIANT: s_trace_collide}),
}
EXEMPT_FROM_SEQUENCES = {
    "hns_sim_trace_points_collide": "reads the velocity and collision_sdf and writes caller-owned arrays only, as hns_sim_trace_points, an operation, does; test_points_collide_gpu holds the sim to a twin",
}


def register():
    """idempotent: the entries join stream_cases.CASES and sequence_cases.EXEMPT"""
    for name, entry in CASES.items():
        sc.CASES.setdefault(name, entry)
    for name, reason in EXEMPT_FROM_SEQUENCES.items():
        sq.EXEMPT.setdefault(name, reason)


register()
