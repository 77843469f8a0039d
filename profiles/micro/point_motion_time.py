#!/usr/bin/env python3
"""Points with a velocity of their own (device.PointMotion.step: hns_point_motion_step, hns_point_motion.hip) on the dense 256^3 grid with n = 2^22 points and 8 steps,
against hns_sim_trace_points_collide at order 1 in mode push on the same points, the same sim and the same lattice SDF. That call's code is the parent commit's: this
change does not touch hns_points_collide.hip. Per step both take one Vec3f sample and one float sample, and six more float samples per push on a hit; the new call
moves 28 instead of 12 bytes per point each way (position, velocity, age), once per call.

For each point set -- in leaf order, and the same points randomly permuted -- six forms alternate rep by rep in this one process, each call bracketed by hipEvents on
the launch stream, the rows restored from copies before every call and outside the bracket:
  trace_push        hns_sim_trace_points_collide(order 1, mode push): the comparator
  free / stick / bounce / kill
                    hns_point_motion_step in each mode: drag 2, gravity (0, -9.8, 0), restitution 0.5, friction 0.25, no age limit. These points are no tracers: they
                    fall some 3 units per second by the last step (35 voxels a step), so they cross leaves, leave the domain and land in the lattice far more often
                    than the comparator's points do -- the shares say how often
  bounce_as_tracer  mode bounce with drag 1e4 and no gravity: v is the gas's velocity to a quarter of a percent after every step, so the points go where the
                    comparator's go and hit what they hit: the like-for-like ratio of the two kernels
Medians of --reps calls with min and max; the first two reps of every form are not counted. Ratios are medians over the median of `trace_push`.

Usage: python profiles/micro/point_motion_time.py [--reps N] [--n POINTS] [--out FILE]
Prints one JSON line and appends it to FILE (default profiles/point_motion_time_256.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT, STEPS = 1.0 / 24.0, 8
COLLIDE = dict(threshold=0.0, skin=1.0 / 16, iterations=3)
SPEC = dict(gravity=(0.0, -9.8, 0.0), drag=2.0, restitution=0.5, friction=0.25, **COLLIDE)
SPEED = 0.5  # standard deviation of the points' starting velocity, in the units of the sim's velocity


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def make_points(origins, n, seed):
    """n points at random offsets inside the domain, point p in leaf p * leaves / n"""
    rng = np.random.default_rng(seed)
    leaf = (np.arange(n, dtype=np.int64) * len(origins)) // n
    return (origins[leaf].astype(np.float64) + rng.uniform(0.0, 8.0, (n, 3))).astype(np.float32)


def lattice_sdf(coords, inv_dx):
    """spheres of radius 3 voxels centred on every leaf corner, in world units"""
    m = ((coords.astype(np.int64) + 4) % 8) - 4
    return ((np.sqrt((m * m).sum(1).astype(np.float64)) - 3.0) / inv_dx).astype(np.float32)


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)
    lib = _lib.load_library()

    def once(fn, before):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def alternating(forms, before, warm=2):
        out = {k: [] for k in forms}
        for rep in range(args.reps + warm):
            for k, fn in forms.items():
                t = once(fn, before)
                if rep >= warm:
                    out[k].append(t)
        return out

    o, R = fields.config_leaves("256")
    vs, N, n = 1.0 / R, len(o) * 512, args.n
    g = api.create_grid_from_leaves(o, vs)
    sim = device.Sim(g, ["collision_sdf"])
    sim.upload({"vel": fields.synthetic_fields(o, R)["vel"], "collision_sdf": lattice_sdf(g.coords(), float(R))})
    ordered = make_points(o, n, 9)
    perm = np.random.default_rng(10).permutation(n)
    rng = np.random.default_rng(11)
    v0 = (SPEED * rng.standard_normal((n, 3))).astype(np.float32)
    line = {"library": os.path.basename(_lib.library_path()), "reps": args.reps, "steps": STEPS, "spec": SPEC, "start_speed": SPEED,
            "config": f"256: {len(o)} leaves, {N} voxels, voxel size 1/{R}; synthetic velocity, dt 1/24; {n} points"}
    motion = sim.point_motion(n)
    xyz, vel, age, status, hit = motion.xyz, motion.vel, motion.age, motion.status, motion.hit
    traced = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    t_status, t_hit = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    push = _lib.hns_point_collision(_lib.HNS_COLLIDE_PUSH, COLLIDE["threshold"], COLLIDE["skin"], COLLIDE["iterations"])
    for name, order in (("leaf_order", None), ("permuted", perm)):
        start = torch.from_numpy(ordered if order is None else ordered[order]).cuda()
        start_v = torch.from_numpy(v0 if order is None else v0[order]).cuda()

        def restore():
            traced.copy_(start), xyz.copy_(start), vel.copy_(start_v), age.zero_()

        def trace_push():
            api._raise(lib.hns_sim_trace_points_collide(sim._ptr, traced.data_ptr(), n, DT, vs, 1, STEPS, C.byref(push), t_status.data_ptr(), t_hit.data_ptr(),
                                                        device.current_stream()))

        def step(mode):
            return lambda: motion.step(sim, n, DT, vs, STEPS, mode, **SPEC)

        def as_tracer():
            motion.step(sim, n, DT, vs, STEPS, "bounce", **{**SPEC, "drag": 1e4, "gravity": (0.0, 0.0, 0.0)})

        forms = {"trace_push": trace_push, "free": step("free"), "stick": step("stick"), "bounce": step("bounce"), "kill": step("kill"), "bounce_as_tracer": as_tracer}
        t = alternating(forms, restore)
        row = {k: {"ms": spread(v)} for k, v in t.items()}
        base = float(np.median(t["trace_push"]))
        for k in forms:
            restore()
            forms[k]()
            torch.cuda.synchronize()
            h, st = (t_hit, t_status) if k == "trace_push" else (hit, status)
            h = h.cpu().numpy()
            row[k]["shares"] = {"pushed_or_bounced": round(float((h & 1 != 0).mean()), 4), "put_back": round(float((h & 2 != 0).mean()), 4),
                                "killed": round(float((h & 4 != 0).mean()), 4), "started_inside": round(float((h & 8 != 0).mean()), 4),
                                "reflected": round(float((h & 16 != 0).mean()), 4), "status_1_at_the_end": round(float(st.float().mean()), 4)}
            if k != "trace_push":
                row[k]["over_trace_push"] = round(float(np.median(t[k])) / base, 3)
        line[name] = row
    motion.close(), sim.close()
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_motion_time_256.jsonl"))
    args = ap.parse_args()
    line = measure(args)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
