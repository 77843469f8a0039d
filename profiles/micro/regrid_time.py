#!/usr/bin/env python3
"""Device regrid (hns_sim_regrid) against the host chain it replaces, at 256^3 with the five fields of the combustion substep (density, fuel, waste,
temperature, flame) + velocity, padding 1 and 8. The sim starts with every voxel active on 32^3 leaves, so both paddings add a ring: 34^3 leaves after.

  device  hipEvent split of the regrid (Sim.regrid_times): candidates | origins to the host + sort + grid tables | masks | field copy, plus the
          wall time of the call; the field copy against its bytes (old leaves read, new leaves written) and against a plain device copy of as many bytes
  host    hns_sim_download -> hns_dilate_leaf_masks -> hns_gather_leaves per field -> new grid -> hns_sim_create -> hns_sim_upload, wall time

Usage: python profiles/micro/regrid_time.py [--reps N] [--out FILE]; prints one JSON line per configuration."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields, leafio  # noqa: E402

NAMES = ["density", "fuel", "waste", "temperature", "flame"]


def copy_floor_ms(nbytes: int, reps: int) -> float:
    """min time of a plain device copy moving nbytes in total (nbytes / 2 read, nbytes / 2 written), inputs evicted from the Infinity Cache"""
    a = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").uniform_()
    b = torch.empty_like(a)
    junk = torch.empty(128 << 20, dtype=torch.float32, device="cuda").uniform_()
    junk2 = torch.empty_like(junk)
    ts = []
    for _ in range(reps):
        junk2.copy_(junk)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        b.copy_(a)
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    R = 256
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + NAMES}
    vs = 1.0 / R
    lines = []
    for p in (1, 8):
        dev, walls = [], []
        for _ in range(args.reps):
            g = api.create_grid_from_leaves(o, vs)
            s = device.Sim(g, NAMES)
            s.upload(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ng = s.regrid(p)
            walls.append((time.perf_counter() - t0) * 1e3)
            dev.append(s.regrid_times())
            n_new = ng.leaf_count()
            s.close()
            g.reset()
            ng.reset()
        host = []
        for _ in range(args.reps):
            g = api.create_grid_from_leaves(o, vs)
            s = device.Sim(g, NAMES)
            s.upload(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = g.voxel_count()
            cur = {"vel": np.empty((n, 3), dtype=np.float32), **{k: np.empty(n, dtype=np.float32) for k in NAMES}}
            s.download(cur)
            dom, dm = leafio.dilate_leaf_masks(o, p, None)
            nxt = {"vel": leafio.gather_leaves(dom, o, cur["vel"], 3, leafio.FILL_ZERO)}
            for k in NAMES:
                nxt[k] = leafio.gather_leaves(dom, o, cur[k], 1, leafio.FILL_ZERO)
            ng = api.create_grid_from_leaves(dom, vs)
            s2 = device.Sim(ng, NAMES)
            s2.set_active_masks(dm)
            s2.upload(nxt)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            s.close(), s2.close()
            g.reset(), ng.reset()
        floats = 3 + len(NAMES)
        moved = 4 * 512 * floats * (len(o) + n_new)  # every old leaf is read (all lie in the new domain), every new leaf written
        floor = copy_floor_ms(moved, args.reps)
        best = min(dev, key=lambda t: sum(t.values()))
        line = {
            "config": f"256^3 S=5 padding={p}", "leaves_before": len(o), "leaves_after": n_new,
            "device_split_ms_best": {k: round(v, 4) for k, v in best.items()},
            "device_split_ms_median": {k: round(float(np.median([t[k] for t in dev])), 4) for k in best},
            "device_wall_ms": {"min": round(min(walls), 3), "median": round(float(np.median(walls)), 3)},
            "field_copy_bytes": moved, "field_copy_TBps": round(moved / (best["fields"] * 1e-3) / 1e12, 3),
            "plain_copy_same_bytes_ms": round(floor, 4), "plain_copy_TBps": round(moved / (floor * 1e-3) / 1e12, 3),
            "floor_6p3TBps_ms": round(moved / 6.3e12 * 1e3, 4),
            "host_chain_ms": {"min": round(min(host), 2), "median": round(float(np.median(host)), 2)},
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
