#!/usr/bin/env python3
"""Points traced against a collision SDF (device.trace_points_collide: hns_dev_trace_points_collide, hns_points_collide.hip) on the dense 256^3 grid with n = 2^22
points, at order 4 with 8 steps, against hns_dev_trace_points on the same points and the same velocity.

For each point set -- in leaf order, and the same points randomly permuted -- five forms alternate rep by rep in this one process, each call bracketed by hipEvents on
the launch stream, the positions restored from a copy before every call and outside the bracket:
  plain             hns_dev_trace_points: the comparator, on the same build
  positive_push     PUSH against an SDF that is positive everywhere: no point ever collides, so the difference to `plain` is the one float sample per step (and the one
                    at the start) plus whatever the larger kernel costs in occupancy
  lattice_stop / lattice_push / lattice_kill
                    the three modes against the lattice of spheres of tests/points_collide_cases.py (radius 3 voxels on every leaf corner, 22 % of the volume inside)
Medians of --reps calls with min and max; the first two reps of every form are not counted. Ratios are medians over the median of `plain`.

Usage: python profiles/micro/points_collide_time.py [--reps N] [--n POINTS] [--out FILE]
Prints one JSON line and appends it to FILE (default profiles/points_collide_time_256.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT, ORDER, STEPS = 1.0 / 24.0, 4, 8
SPEC = dict(threshold=0.0, skin=1.0 / 16, iterations=2)


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
    vs, inv_dx, N, n = 1.0 / R, float(R), len(o) * 512, args.n
    g = api.create_grid_from_leaves(o, vs)
    u = torch.from_numpy(fields.synthetic_fields(o, R)["vel"]).cuda()
    lattice = torch.from_numpy(lattice_sdf(g.coords(), inv_dx)).cuda()
    positive = lattice.abs() + 0.01
    ordered = make_points(o, n, 9)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)]}
    line = {"library": os.path.basename(_lib.library_path()), "reps": args.reps, "order": ORDER, "steps": STEPS, "spec": SPEC,
            "config": f"256: {len(o)} leaves, {N} voxels, voxel size 1/{R}; synthetic velocity, dt 1/24; {n} points"}
    for name, pts in sets.items():
        start = torch.from_numpy(pts).cuda()
        xyz = torch.empty_like(start)
        status, hit = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

        def collide(sdf, mode):
            return lambda: device.trace_points_collide(g, u, sdf, xyz, DT, inv_dx, ORDER, STEPS, mode=mode, status=status, hit=hit, **SPEC)

        forms = {"plain": lambda: device.trace_points(g, u, xyz, DT, inv_dx, ORDER, STEPS, status), "positive_push": collide(positive, "push"),
                 "lattice_stop": collide(lattice, "stop"), "lattice_push": collide(lattice, "push"), "lattice_kill": collide(lattice, "kill")}
        t = alternating(forms, lambda: xyz.copy_(start))
        row = {k: {"ms": spread(v)} for k, v in t.items()}
        base = float(np.median(t["plain"]))
        for k in forms:
            if k != "plain":
                row[k]["over_plain"] = round(float(np.median(t[k])) / base, 3)
                xyz.copy_(start)
                forms[k]()
                h = hit.cpu().numpy()
                row[k]["shares"] = {"pushed": round(float((h & 1 != 0).mean()), 4), "put_back": round(float((h & 2 != 0).mean()), 4),
                                    "killed": round(float((h & 4 != 0).mean()), 4), "started_inside": round(float((h & 8 != 0).mean()), 4),
                                    "alive_inside_at_the_end": round(float(status.float().mean()), 4)}
        line[name] = row
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_collide_time_256.jsonl"))
    args = ap.parse_args()
    line = measure(args)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
