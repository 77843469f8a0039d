#!/usr/bin/env python3
"""Sampling fields at points and tracing points through the velocity (hns_dev_sample_points / hns_dev_trace_points, hns_points.hip) on the dense 256^3 grid:
n = 2^22 points at random offsets inside the domain, (a) in leaf order -- point p lies in leaf p * leaves / n, the order a caller gets who emits from the
fields -- and (b) the same points randomly permuted. The velocity is the synthetic one (fields.synthetic_fields, amplitude 96 voxels/s): at dt = 1/24
displacements of about 2 voxels per step, up to 5 in the plume.

Runs: samples of 1, 4 and 8 float fields plus the velocity in one call; traces at order 1, 2 and 4 with steps 1 and 8 (every trace starts from the same
positions: they are copied back first, outside the timed stretch). Each figure is the median of --reps launches, each bracketed by hipEvents on the launch
stream, with min and max beside it: the spread a difference has to exceed. The yardstick measured in the same process is k_advect_vector_n
(hns_dev_advect_vector) on the same grid and velocity, in ns per voxel, set beside ns per point and sample (a trace of order o and s steps takes o * s
samples of the velocity, the status lookup not counted); nothing is gated on it.

One process measures ONE build of the library (HNS_LIBRARY, hnanosolver_amd/_lib.py). --ab A.so B.so alternates two builds, each run a fresh child
process of this script (--only trace), A B A B ..., --rounds times each, in one call on one box, as profiles/README.md describes for every A/B; a digest
of the traced positions shows that the two builds computed the same words.

Usage: python profiles/micro/points_time.py [--reps N] [--n POINTS] [--only trace|sample] [--label TEXT] [--out FILE]
       python profiles/micro/points_time.py --ab A.so B.so [--rounds K] [--reps N] [--out FILE]
Prints one JSON line per process and appends it to FILE."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT = 1.0 / 24.0
ORDERS, STEPS, FLOATS = (1, 2, 4), (1, 8), (1, 4, 8)


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def make_points(origins, n, seed):
    """n points at random offsets inside the domain, point p in leaf p * leaves / n"""
    rng = np.random.default_rng(seed)
    leaf = (np.arange(n, dtype=np.int64) * len(origins)) // n
    return (origins[leaf].astype(np.float64) + rng.uniform(0.0, 8.0, (n, 3))).astype(np.float32)


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)

    def timed(fn, before=None):
        out = []
        for rep in range(args.reps + 3):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                out.append(a.elapsed_time(b))
        return out

    o, R = fields.config_leaves("256")
    vs, inv_dx, N, n = 1.0 / R, float(R), len(o) * 512, args.n
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, vs)
    u = torch.from_numpy(f["vel"]).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    names = ["density", "temperature", "fuel", "waste", "flame"]
    phi = [torch.from_numpy(f[k]).cuda() for k in names] + [torch.randn(N, device="cuda", generator=gen) for _ in range(max(FLOATS) - len(names))]
    ordered = make_points(o, n, 9)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)]}
    line = {"library": os.path.basename(_lib.library_path()), "label": args.label, "reps": args.reps,
            "config": f"256: {len(o)} leaves, {N} voxels, voxel size 1/{R}; synthetic velocity, dt 1/24; {n} points"}
    adv = torch.empty_like(u)
    t = timed(lambda: device.advect_vector(g, u, adv, DT, inv_dx))
    line["advect_vector_ms"] = spread(t)
    line["advect_vector_ns_per_voxel"] = round(1e6 * float(np.median(t)) / N, 4)
    del adv
    digest = hashlib.sha1()
    for name, pts in sets.items():
        start = torch.from_numpy(pts).cuda()
        res = line[name] = {}
        if args.only in (None, "sample"):
            outs = [torch.empty(n, device="cuda") for _ in range(max(FLOATS))] + [torch.empty((n, 3), device="cuda")]
            for S in FLOATS:
                t = timed(lambda: device.sample_points(g, phi[:S] + [u], start, outs[:S] + outs[-1:]))
                res[f"sample_{S}_floats_and_velocity"] = {"ms": spread(t), "ns_per_point_and_field": round(1e6 * float(np.median(t)) / (n * (S + 1)), 4)}
            del outs
        if args.only in (None, "trace"):
            xyz, status = torch.empty_like(start), torch.empty(n, dtype=torch.uint8, device="cuda")
            for order in ORDERS:
                for steps in STEPS:
                    t = timed(lambda: device.trace_points(g, u, xyz, DT, inv_dx, order, steps, status), before=lambda: xyz.copy_(start))
                    res[f"trace_order{order}_steps{steps}"] = {"ms": spread(t), "ns_per_point_and_sample": round(1e6 * float(np.median(t)) / (n * order * steps), 4),
                                                               "inside_at_the_end": round(float(status.float().mean()), 4)}
                    digest.update(xyz.cpu().numpy().tobytes() + status.cpu().numpy().tobytes())
    line["traced_words_sha1"] = digest.hexdigest()[:16]
    return line


def emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--only", choices=("trace", "sample"), default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", nargs=2, metavar=("A.so", "B.so"), default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    args = ap.parse_args()
    if not args.ab:
        emit(measure(args), args.out)
        return 0
    # the parent never opens the GPU: every run is a fresh child, and the first one that fails ends the series
    for rnd in range(args.rounds):
        for which, lib in zip("AB", args.ab):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", "trace", "--reps", str(args.reps), "--n", str(args.n), "--label", f"{which} round {rnd}"]
            r = subprocess.run(cmd, env={**os.environ, "HNS_LIBRARY": os.path.abspath(lib)}, capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode or 1
            emit(json.loads(r.stdout.strip().splitlines()[-1]), args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
