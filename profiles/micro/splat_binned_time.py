#!/usr/bin/env python3
"""Point values into fields through a leaf order (device.PointOrder.splat: hns_point_order_splat, hns_splat_binned.hip) against the plain call (device.splat_points:
hns_dev_splat_points) on the dense 256^3 grid.

Point sets of n = 2^22, as profiles/micro/point_order_time.py makes them: (a) leaf_order -- point p lies in leaf p * leaves / n --, (b) permuted -- the same points in
random order --, (c) ball -- an emitter ball of radius 3 voxels on a leaf corner: eight leaves hold every point, the case one workgroup per destination leaf is worst at.

Rows: one float and the velocity, trilinear; one float, radial at r = 2 and r = 4. For every set and row three forms alternate rep by rep in this one process, each call
bracketed by hipEvents on the launch stream:
  plain         hns_dev_splat_points on the points as the set holds them (the comparator: never a figure from a document)
  ordered       the ordered call alone, on ranked rows -- a caller that keeps its points and attributes in sorted order
  sort_gather_ordered   sort + gather of positions and values + the ordered call -- a caller whose points arrive unordered
Medians of --reps calls with min and max. A row whose calls take longer than --slow-ms runs --slow-reps reps, and says so. `level_ab`: the ordered trilinear call after a
sort by leaf against after a sort by voxel (the same kernel: what differs is the order of a leaf's points, and with it how the LDS adds of a wave collide).

Usage: python profiles/micro/splat_binned_time.py [--reps N] [--n POINTS] [--out FILE] [--table FILE]
Prints one JSON line per point set and appends them to FILE; writes the short table to the --table file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")


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

    def alternating(forms):
        """{name: fn} -> ({name: [ms]}, reps): the forms in turn within every rep; one untimed round first, whose times pick the number of reps"""
        probe = max(once(fn) for fn in forms.values())
        reps, warm = (args.slow_reps, 0) if probe > args.slow_ms else (args.reps, 2)
        out = {k: [] for k in forms}
        for rep in range(reps + warm):
            for k, fn in forms.items():
                t = once(fn)
                if rep >= warm:
                    out[k].append(t)
        return out, reps

    o, R = fields.config_leaves("256")
    L, n = len(o), args.n
    N = L * 512
    g = api.create_grid_from_leaves(o, 1.0 / R)
    rng = np.random.default_rng(9)
    leaf = (np.arange(n, dtype=np.int64) * L) // n
    ordered = (o[leaf].astype(np.float64) + rng.uniform(0.0, 8.0, (n, 3))).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d *= (3.0 * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    ball = (o[L // 2].astype(np.float64) + 8.0 + d).astype(np.float32)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)], "ball": ball}
    sets = {k: v for k, v in sets.items() if k in args.sets.split(",")}
    vals, vvals = torch.randn(n, device="cuda"), torch.randn((n, 3), device="cuda")
    target, target3 = torch.zeros(N, device="cuda"), torch.zeros((N, 3), device="cuda")
    rows = {
        "trilinear_1_float": ([target], [vals], {}),
        "trilinear_velocity": ([target3], [vvals], {}),
        "radial_r2_1_float": ([target], [vals], dict(kernel="radial", radius=2.0)),
        "radial_r4_1_float": ([target], [vals], dict(kernel="radial", radius=4.0)),
    }
    po = device.PointOrder(g, n)
    lines = []
    for name, host in sets.items():
        x = torch.from_numpy(host).cuda()
        line = {"set": name, "library": os.path.basename(_lib.library_path()), "config": f"256: {L} leaves, {N} voxels; {n} points", "reps": args.reps}
        xs = torch.empty_like(x)
        for row, (dst, src, spec) in rows.items():
            ranked = [torch.empty_like(v) for v in src]

            def sort_gather():
                po.sort(x, "voxel")
                po.gather(x, xs)
                for v, r in zip(src, ranked):
                    po.gather(v, r)

            def full():
                sort_gather()
                po.splat(dst, xs, ranked, rows="ranked", **spec)

            sort_gather()
            t, reps = alternating({"plain": lambda: device.splat_points(g, dst, x, src, **spec), "ordered": lambda: po.splat(dst, xs, ranked, rows="ranked", **spec),
                                   "sort_gather_ordered": full})
            line[row] = {k: spread(v) for k, v in t.items()}
            line[row]["reps"] = reps
            line[row]["plain_over_ordered"] = round(float(np.median(t["plain"]) / np.median(t["ordered"])), 3)
            line[row]["plain_over_sort_gather_ordered"] = round(float(np.median(t["plain"]) / np.median(t["sort_gather_ordered"])), 3)
        # the ordered trilinear call after a sort by leaf and after a sort by voxel
        po_leaf = device.PointOrder(g, n).sort(x, "leaf")
        xl, vl = po_leaf.gather(x), po_leaf.gather(vals)
        po.sort(x, "voxel")
        po.gather(x, xs)
        vv = po.gather(vals)
        t, reps = alternating({"leaf": lambda: po_leaf.splat([target], xl, [vl], rows="ranked"), "voxel": lambda: po.splat([target], xs, [vv], rows="ranked")})
        line["level_ab"] = {k: spread(v) for k, v in t.items()}
        line["level_ab"]["reps"] = reps
        po_leaf.close()
        del x, xs, xl, vl, vv
        print(json.dumps(line), flush=True)
        lines.append(line)
    po.close()
    return lines


def table(lines):
    out = [f"ordered splat against the plain call on {lines[0]['config']}; medians in ms (min .. max)", ""]
    fmt = lambda m: f"{m['median']:9.3f} ({m['min']:.3f} .. {m['max']:.3f})"
    for line in lines:
        for row, r in line.items():
            if not isinstance(r, dict) or "plain" not in r:
                continue
            out.append(f"{line['set']:10s} {row:20s} plain {fmt(r['plain'])}  ordered {fmt(r['ordered'])}  sort+gather+ordered {fmt(r['sort_gather_ordered'])}  "
                       f"plain/ordered {r['plain_over_ordered']:.2f}  plain/(sort+gather+ordered) {r['plain_over_sort_gather_ordered']:.2f}  reps {r['reps']}")
        ab = line["level_ab"]
        out.append(f"{line['set']:10s} trilinear_1_float, ordered after a sort by leaf {fmt(ab['leaf'])}, by voxel {fmt(ab['voxel'])}")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=150.0)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--sets", default="leaf_order,permuted,ball")
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    lines = measure(args)
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    if args.table:
        with open(args.table, "w") as fh:
            fh.write(table(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
