#!/usr/bin/env python3
"""End-of-frame deactivation (hns_sim_deactivate) at 256^3: 32^3 leaves, the five combustion fields + velocity, velocity and density tested. The
density tolerance (1.0, the blob's peak) keeps every density within, so the velocity is read for every active voxel too: 16 bytes per active voxel,
the most the kernel reads. Two mask states, reset before every call:

  all_active  every bit set (the masks are read, as in a frame chain)
  half_zero   every second leaf (grid order) has an all-zero mask: its rounds load nothing

Each call is bracketed by hipEvents on the stream it runs on (the table launch + the ballot kernel). In the same run, alternated with the calls: a
device-to-device copy (torch copy_) of as many bytes as the all-active call reads. The device masks and counts are checked once against the host
mirror (hns_deactivate_leaf_masks) for both states.

Usage: python profiles/micro/deactivate_time.py [--reps N] [--out FILE]; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields, leafio  # noqa: E402

NAMES = ["density", "fuel", "waste", "temperature", "flame"]
TOL = {"density": 1.0}
VEL_TOL = 1e-3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    R = 256
    o = fields.dense_leaves(R)
    n_leaves = len(o)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + NAMES}
    g = api.create_grid_from_leaves(o, 1.0 / R)
    s = device.Sim(g, NAMES)
    s.upload(st)
    masks = {"all_active": np.full((n_leaves, 64), 0xFF, dtype=np.uint8)}
    half = masks["all_active"].copy()
    half[::2] = 0
    masks["half_zero"] = half
    checks = {}
    for name, m in masks.items():  # correctness at this size, once
        s.set_active_masks(m)
        counts = s.deactivate(TOL, VEL_TOL, counts=True)
        want, want_counts = leafio.deactivate_masks(m, {"density": (st["density"], TOL["density"])}, (st["vel"], VEL_TOL))
        assert np.array_equal(s.active_masks(), want) and counts == want_counts, name
        checks[name] = {"active_voxels_after": counts[0], "active_leaves_after": counts[1]}
    read_bytes = {k: int(np.unpackbits(m).sum()) * 16 + m.nbytes for k, m in masks.items()}  # 16 B per active voxel + the masks
    nbytes = read_bytes["all_active"]
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    times = {k: [] for k in masks}
    copy = []
    for rep in range(args.reps + 3):
        for name, m in masks.items():
            s.set_active_masks(m)
            torch.cuda.synchronize()
            t = timed(lambda: s.deactivate(TOL, VEL_TOL))
            if rep >= 3:
                times[name].append(t)
        t = timed(lambda: dst.copy_(src))
        if rep >= 3:
            copy.append(t)
    line = {
        "config": f"256^3 ({n_leaves} leaves), S=5 + velocity, tested: velocity (tol {VEL_TOL}) and density (tol {TOL['density']}: always within)",
        "reps": args.reps,
        "deactivate_ms": {k: stats(v) for k, v in times.items()},
        "deactivate_read_bytes": read_bytes,
        "deactivate_read_TBps_at_median": {k: round(read_bytes[k] / (np.median(v) * 1e-3) / 1e12, 3) for k, v in times.items()},
        "d2d_copy_bytes": nbytes,
        "d2d_copy_ms": stats(copy),
        "d2d_copy_read_plus_write_TBps_at_median": round(2 * nbytes / (np.median(copy) * 1e-3) / 1e12, 3),
        "checked_against_host_mirror": checks,
    }
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    s.close()


if __name__ == "__main__":
    main()
