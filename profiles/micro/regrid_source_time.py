#!/usr/bin/env python3
"""Sourced device regrid (hns_sim_regrid_sourced) against the unsourced one and against the host chain it replaces, at 256^3 with the five fields of
the combustion substep (density, fuel, waste, temperature, flame) + velocity, padding 1. The sim starts with every voxel active on 32^3 leaves; the
sources (velocity, density, temperature, fuel) cover a 64^3-voxel emitter (8^3 = 512 leaves), half of it beyond the +x face of the domain.

  sourced    hipEvent split of the regrid (Sim.regrid_times): candidates | origins to the host + sort + grid tables (the source uploads are issued
             there) | masks | fields, and the wall time of the call; the source bytes that cross PCIe
  unsourced  hns_sim_regrid on the same state, wall time, alternated with the sourced call
  host       hns_sim_download -> hns_add_leaves per source -> hns_dilate_leaf_masks -> hns_gather_leaves per field -> new grid -> hns_sim_create ->
             hns_sim_upload, wall time
  pageable   how long a pageable hipMemcpyAsync of the source bytes keeps the host (call return) against its completion (after the stream sync):
             whether the source uploads can overlap the host sort at all

Usage: python profiles/micro/regrid_source_time.py [--reps N] [--out FILE]; prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields, leafio  # noqa: E402

NAMES = ["density", "fuel", "waste", "temperature", "flame"]


def emitter(R):
    lat = np.stack(np.meshgrid(np.arange(-4, 4), np.arange(-4, 4), np.arange(-4, 4), indexing="ij"), -1).reshape(-1, 3)
    o = ((lat + np.array([R // 8, R // 16, R // 16])) * 8).astype(np.int32)  # x leaves [R/8 - 4, R/8 + 4): half outside [0, R)
    rng = np.random.default_rng(7)
    src = {"vel": (o, None, (rng.random((len(o) * 512, 3)) * np.float32(0.5)).astype(np.float32))}
    for name in ("density", "temperature", "fuel"):
        src[name] = (o, None, rng.random(len(o) * 512).astype(np.float32))
    return src


def pageable_copy_ms(nbytes: int, reps: int):
    """(min ms until hipMemcpyAsync returns, min ms until the copy is complete) for a pageable host buffer of nbytes"""
    with open("/proc/self/maps") as f:  # the HIP runtime this process already runs on (torch's and libhns's), not a second copy
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    dst = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    src = np.random.default_rng(1).random(nbytes // 4).astype(np.float32)
    torch.cuda.synchronize()
    ret, done = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.ctypes.data, nbytes, 1, None) == 0  # hipMemcpyHostToDevice, null stream
        t1 = time.perf_counter()
        assert hip.hipStreamSynchronize(None) == 0
        t2 = time.perf_counter()
        ret.append((t1 - t0) * 1e3)
        done.append((t2 - t0) * 1e3)
    return min(ret), min(done)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    R, p = 256, 1
    o = fields.dense_leaves(R)
    st = fields.synthetic_fields(o, R)
    st = {k: st[k] for k in ["vel"] + NAMES}
    vs = 1.0 / R
    src = emitter(R)
    src_bytes = sum(v.nbytes + so.size * 4 + (0 if sm is None else sm.nbytes) for so, sm, v in src.values())
    dev, walls, plain_walls = [], [], []
    n_plain = n_new = 0
    for _ in range(args.reps):
        for sourced in (False, True):
            g = api.create_grid_from_leaves(o, vs)
            s = device.Sim(g, NAMES)
            s.upload(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ng = s.regrid(p, None, src if sourced else None)
            wall = (time.perf_counter() - t0) * 1e3
            if sourced:
                walls.append(wall)
                dev.append(s.regrid_times())
                n_new = ng.leaf_count()
            else:
                plain_walls.append(wall)
                n_plain = ng.leaf_count()
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
        vo, vm, vv = leafio.add_leaves((o, None, cur["vel"]), src["vel"], 3)
        summed = {k: leafio.add_leaves((o, None, cur[k]), src[k], 1) for k in NAMES if k in src}
        dom, dm = leafio.dilate_leaf_masks(vo, p, vm)
        nxt = {"vel": leafio.gather_leaves(dom, vo, vv, 3, leafio.FILL_ZERO)}
        for k in NAMES:
            so, _, sv = summed[k] if k in summed else (o, None, cur[k])
            nxt[k] = leafio.gather_leaves(dom, so, sv, 1, leafio.FILL_ZERO)
        ng = api.create_grid_from_leaves(dom, vs)
        s2 = device.Sim(ng, NAMES)
        s2.set_active_masks(dm)
        s2.upload(nxt)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        assert len(dom) == n_new
        s.close(), s2.close()
        g.reset(), ng.reset()
    ret_ms, done_ms = pageable_copy_ms(sum(v.nbytes for _, _, v in src.values()), args.reps)
    best = min(dev, key=lambda t: sum(t.values()))
    med = lambda xs: round(float(np.median(xs)), 3)  # noqa: E731
    line = {
        "config": f"256^3 S=5 padding={p}, sources vel+density+temperature+fuel on {len(src['vel'][0])} leaves (half outside)",
        "leaves_before": len(o), "leaves_after_unsourced": n_plain, "leaves_after_sourced": n_new,
        "source_bytes_uploaded": int(src_bytes),
        "sourced_device_split_ms_best": {k: round(v, 4) for k, v in best.items()},
        "sourced_device_split_ms_median": {k: round(float(np.median([t[k] for t in dev])), 4) for k in best},
        "sourced_wall_ms": {"min": round(min(walls), 3), "median": med(walls)},
        "unsourced_wall_ms": {"min": round(min(plain_walls), 3), "median": med(plain_walls)},
        "sourced_minus_unsourced_ms": {"min": round(min(walls) - min(plain_walls), 3), "median": round(med(walls) - med(plain_walls), 3)},
        "host_chain_ms": {"min": round(min(host), 2), "median": round(float(np.median(host)), 2)},
        "pageable_h2d_of_source_values_ms": {"call_returns": round(ret_ms, 3), "complete": round(done_ms, 3)},
    }
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
