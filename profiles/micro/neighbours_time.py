#!/usr/bin/env python3
"""Point neighbourhoods through a leaf order (device.PointOrder.neighbours: hns_point_order_neighbours, hns_neighbours.hip) on the dense 256^3 grid: the time of the cell
table and of the query, with the sort of the same points and the radial splat at r = h for scale.

Point sets of n = 2^22: (a) spread -- uniform over the 256^3 grid, a quarter of a point per voxel --, (b) block -- uniform over an 80^3 block in the middle of it, 8.2 per
voxel. Radii h = 0.5, 1 and 2; all three outputs; ranked rows (positions gathered into sorted order once, outside the timed calls). For every set and radius the forms
alternate rep by rep in this one process, each call bracketed by hipEvents on the launch stream:
  sort          hns_point_order_sort at voxel level
  sort_table    the sort and hns_point_order_cells behind it (the table is rebuilt by the first call behind a sort): table = the difference of the two medians
  query         hns_point_order_neighbours on a fresh table
  splat_radial  hns_dev_splat_points, radial at r = h, one float field, the same ranked points (k_splat_radial: a kernel of the same shape that adds into voxels)
candidate_pairs: the (i, j) the query examines -- for every point that takes part the points in the cells of its box, itself excluded --, counted here from a
summed-volume table of the per-voxel counts and never by the kernel. neighbour_pairs: the sum of the counts the query returned. Medians of --reps calls with min and max.

Usage: python profiles/micro/neighbours_time.py [--reps N] [--n POINTS] [--out FILE]
Prints one JSON line per point set and radius and appends them to FILE."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
RADII = (0.5, 1.0, 2.0)


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def candidate_pairs(torch, x, h, R):
    """sum over the points of the points in the cells floorf(x - h) .. floorf(x + h) per axis, itself excluded; every point lies inside the dense R^3 grid"""
    cell = torch.floor(x).long()
    counts = torch.zeros(R * R * R, dtype=torch.int64, device=x.device)
    counts.index_add_(0, (cell[:, 0] * R + cell[:, 1]) * R + cell[:, 2], torch.ones(len(x), dtype=torch.int64, device=x.device))
    S = torch.zeros((R + 1, R + 1, R + 1), dtype=torch.int64, device=x.device)
    S[1:, 1:, 1:] = counts.view(R, R, R).cumsum(0).cumsum(1).cumsum(2)
    lo = torch.floor(x - h).long().clamp(0, R - 1)
    hi = torch.floor(x + h).long().clamp(0, R - 1) + 1
    total = torch.zeros(len(x), dtype=torch.int64, device=x.device)
    for c in range(8):
        pick = [hi[:, a] if c >> a & 1 else lo[:, a] for a in range(3)]
        sign = -1 if (3 - bin(c).count("1")) % 2 else 1
        total += sign * S[pick[0], pick[1], pick[2]]
    return int((total - 1).sum())


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

    def alternating(forms):
        out = {k: [] for k in forms}
        for rep in range(args.reps + 2):  # two untimed rounds first
            for k, fn in forms.items():
                t = once(fn)
                if rep >= 2:
                    out[k].append(t)
        return out

    o, R = fields.config_leaves("256")
    L, n = len(o), args.n
    N = L * 512
    g = api.create_grid_from_leaves(o, 1.0 / R)
    rng = np.random.default_rng(21)
    sets = {"spread": rng.uniform(0.0, float(R), (n, 3)).astype(np.float32), "block": rng.uniform(88.0, 168.0, (n, 3)).astype(np.float32)}
    sets = {k: np.minimum(v, np.nextafter(np.float32(R), np.float32(0))) for k, v in sets.items() if k in args.sets.split(",")}
    vals, target = torch.randn(n, device="cuda"), torch.zeros(N, device="cuda")
    po = device.PointOrder(g, n)
    lines = []
    for name, host in sets.items():
        x = torch.from_numpy(host).cuda()
        po.sort(x, "voxel")
        xs = po.gather(x)
        out = {"count": torch.empty(n, dtype=torch.int32, device="cuda"), "density": torch.empty(n, device="cuda"), "push": torch.empty((n, 3), device="cuda")}
        for h in RADII:

            def sort_table():
                po.sort(x, "voxel")
                po.cell_start

            forms = {"sort": lambda: po.sort(x, "voxel"), "sort_table": sort_table, "query": lambda: po.neighbours(xs, h, rows="ranked", **out),
                     "splat_radial": lambda: device.splat_points(g, [target], xs, [vals], kernel="radial", radius=h)}
            t = alternating(forms)
            cand, found = candidate_pairs(torch, xs, h, R), int(out["count"].long().sum())
            q = float(np.median(t["query"]))
            line = {"set": name, "radius": h, "library": os.path.basename(_lib.library_path()), "config": f"256: {L} leaves, {N} voxels; {n} points", "reps": args.reps,
                    **{k: spread(v) for k, v in t.items()}, "table_ms": round(float(np.median(t["sort_table"]) - np.median(t["sort"])), 4),
                    "candidate_pairs": cand, "neighbour_pairs": found, "candidate_pairs_per_s": round(cand / (q * 1e-3), 0), "neighbour_pairs_per_s": round(found / (q * 1e-3), 0),
                    "query_over_sort": round(q / float(np.median(t["sort"])), 3), "query_over_splat_radial": round(q / float(np.median(t["splat_radial"])), 3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del x, xs
    po.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--sets", default="spread,block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = measure(args)
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
