#!/usr/bin/env python3
"""advect_scalar over S fields: one hns_dev_advect_scalar_multi call (one back-trace for all of them) against S hns_dev_advect_scalar launches, the path
AdvectIndexGrid took before. Input per config: dense-active or plume leaves, the synthetic fields, and the velocity a core substep of 50 iterations
leaves (the headline's). Per S in {1, 2, 4, 8} the two legs alternate, each bracketed by hipEvents on the launch stream, all in one process; the
outputs of the two legs are compared as 32-bit words first.

Per leg: min / median / max over the pairs -- the spread of repeated runs of one leg in the same call is what a difference has to exceed. Per S: the
ratio of the medians, in how many pairs the one call was the faster leg, and the largest per-pair ratio.

Usage: python profiles/micro/advect_multi_time.py [--configs 256,128,plume1024] [--reps N] [--label TEXT] [--out FILE]; prints one JSON line per config
and appends them to FILE."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields  # noqa: E402

S_LIST = (1, 2, 4, 8)
ITERS, DT = 50, 1.0 / 24.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def headline_velocity(g, f, vs):
    """the velocity after one core substep: what advect_scalars of the headline workload reads"""
    s = device.Sim(g, ["density"])
    s.upload({"vel": f["vel"], "density": f["density"]})
    s.core_substep(ITERS, DT, vs)
    vel = np.empty_like(f["vel"])
    s.download({"vel": vel})
    s.close()
    return vel


def measure(config, reps, label):
    o, R = fields.config_leaves(config)
    vs, inv_dx = 1.0 / R, float(R)
    N = len(o) * 512
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, vs)
    u = torch.from_numpy(headline_velocity(g, f, vs)).cuda()
    names = ["density", "temperature", "fuel", "waste", "flame"]
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = [torch.from_numpy(f[n]).cuda() for n in names] + [torch.randn(N, device="cuda", generator=gen) for _ in range(max(S_LIST) - len(names))]
    one, many = [torch.empty_like(p) for p in src], [torch.empty_like(p) for p in src]

    def singles(S):
        for i in range(S):
            device.advect_scalar(g, u, src[i], one[i], DT, inv_dx)

    def multi(S):
        device.advect_scalar_multi(g, u, src[:S], many[:S], DT, inv_dx)

    legs = {}
    for S in S_LIST:
        singles(S), multi(S)
        torch.cuda.synchronize()
        same = all(torch.equal(one[i].view(torch.int32), many[i].view(torch.int32)) for i in range(S))
        t = {"singles": [], "multi": []}
        for rep in range(reps + 3):
            a, b = timed(lambda: singles(S)), timed(lambda: multi(S))
            if rep >= 3:
                t["singles"].append(a), t["multi"].append(b)
        ratios = [b / a for a, b in zip(t["singles"], t["multi"])]
        legs[str(S)] = {
            "singles_ms": spread(t["singles"]),
            "multi_ms": spread(t["multi"]),
            "multi_over_singles_at_median": round(float(np.median(t["multi"]) / np.median(t["singles"])), 4),
            "pairs_multi_faster": int(sum(r < 1.0 for r in ratios)),
            "largest_pair_ratio": round(max(ratios), 4),
            "outputs_equal_as_words": bool(same),
        }
    return {"config": f"{config}: {len(o)} leaves, {N} voxels, voxel size 1/{R}; velocity after one core substep of {ITERS} iterations", "label": label, "pairs": reps,
            "advect_form": "narrow (32-bit addressed)", "S": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="256,128,plume1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for config in args.configs.split(","):
        line = measure(config, args.reps, args.label)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
