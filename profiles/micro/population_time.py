#!/usr/bin/env python3
"""Birth and death of points (device.PointPopulation: hns_point_population_*, hns_population.hip) on the dense 256^3 grid with n = 2^22 points.

(a) death: select + compact of xyz (12-byte rows) at half kept and at 1/16 kept, against two baselines. For every share three forms alternate rep by rep in this one
    process, each call bracketed by hipEvents on the launch stream:
      select_compact   PointPopulation.select(flags) + compact(xyz, fill = NaN): no host wait
      gather           hns_point_order_gather of the same rows on the same build through a permutation made beforehand: the same bytes moved plus a permutation read,
                       and nothing of what makes the permutation (the comparator: never a figure from a document)
      torch_mask       x[keep.bool()], what a user does today: its host wait is inside the bracket (the result's length is data)
(b) birth: Sim.birth from a field that bears about 2^22 points, against its byte floor: 4 B per voxel read, twice for the two passes, plus 16 B per birth written (xyz and
    voxel), over the 6.3 TB/s a streaming kernel achieves on this part.
Medians of --reps calls with min and max; the first two reps of every row are not counted.

Usage: python profiles/micro/population_time.py [--reps N] [--n POINTS] [--out FILE]
Prints one JSON line and appends it to FILE (default profiles/population_time_256.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
ACHIEVABLE_TBS = 6.3


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def alternating(forms, warm=2):
        out = {k: [] for k in forms}
        for rep in range(args.reps + warm):
            for k, fn in forms.items():
                t = once(fn)
                if rep >= warm:
                    out[k].append(t)
        return out

    o, R = fields.config_leaves("256")
    L, n = len(o), args.n
    N = L * 512
    g = api.create_grid_from_leaves(o, 1.0 / R)
    rng = np.random.default_rng(9)
    x = torch.from_numpy((rng.random((n, 3)) * 256.0).astype(np.float32)).cuda()
    line = {"library": os.path.basename(_lib.library_path()), "config": f"256: {L} leaves, {N} voxels; {n} points", "reps": args.reps}
    pop = device.PointPopulation(g, n)
    po = device.PointOrder(g, n).sort(x, "leaf")  # any permutation will do for the gather: this one is made once, outside every bracket
    dst, gathered = torch.empty_like(x), torch.empty_like(x)
    for name, share in (("half_kept", 0.5), ("sixteenth_kept", 1.0 / 16.0)):
        flags = torch.from_numpy((rng.random(n) < share).astype(np.uint8)).cuda()

        def select_compact():
            pop.select(flags)
            pop.compact(x, dst, fill=float("nan"))

        t = alternating({"select_compact": select_compact, "gather": lambda: po.gather(x, gathered), "torch_mask": lambda: x[flags.bool()]})
        row = {k: spread(v) for k, v in t.items()}
        row["kept"] = pop.counts()[0]
        row["select_compact_over_gather"] = round(float(np.median(t["select_compact"]) / np.median(t["gather"])), 3)
        row["torch_mask_over_select_compact"] = round(float(np.median(t["torch_mask"]) / np.median(t["select_compact"])), 3)
        t = alternating({"select": lambda: pop.select(flags), "compact": lambda: pop.compact(x, dst, fill=float("nan"))})
        row["select"], row["compact"] = spread(t["select"]), spread(t["compact"])
        line[name] = row
    po.close()
    # (b) a field uniform in 0 .. 1 with rate 1, K = 1: half of the voxels bear one point, 2^23 births at 256^3; the rate is scaled to about n
    names = ["flame"]
    sim = device.Sim(g, names)
    flame = rng.random(N).astype(np.float32)
    sim.upload({"vel": np.zeros((N, 3), dtype=np.float32), "flame": flame})
    rate = float(np.float32(2.0 * n / N))
    rows = 2 * n
    xyz, voxel = torch.empty((rows, 3), device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")
    born = sim.point_population(0)
    bear = lambda: sim.birth(born, "flame", xyz, voxel, threshold=0.0, rate=rate, max_per_voxel=1, seed=7, fill=False)
    t = alternating({"birth_sim": bear})
    live, wanted = born.counts()
    floor_ms = (2 * 4 * N + 16 * live) / (ACHIEVABLE_TBS * 1e12) * 1e3
    line["birth"] = {"birth_sim": spread(t["birth_sim"]), "births": live, "wanted": wanted, "byte_floor_ms": round(floor_ms, 4),
                     "over_byte_floor": round(float(np.median(t["birth_sim"])) / floor_ms, 3), "achievable_tb_s": ACHIEVABLE_TBS}
    born.close(), pop.close(), sim.close()
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_time_256.jsonl"))
    args = ap.parse_args()
    line = measure(args)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
