#!/usr/bin/env python3
"""Point values added into fields (hns_dev_splat_points, hns_splat.hip) on the dense 256^3 grid: n = 2^22 points at random offsets inside the domain, (a) in leaf
order -- point p lies in leaf p * leaves / n -- and (b) the same points randomly permuted; the point sets of profiles/micro/points_time.py.

Channel sets: one float field (1 channel), the velocity (3), four float fields and the velocity (7: two launches of the pair k_splat_points + k_splat_finish). Each
figure is the median of --reps calls, each bracketed by hipEvents on the launch stream, with min and max beside it. The yardstick, measured beside every figure in the
same process, is hns_dev_sample_points (k_sample_points) for the same points and the same fields: the transpose -- the same cell work, loads where this has atomics.
`splat_over_sample` is the ratio of the two medians; nothing is gated on it. The fields keep what the repetitions add (values of unit size: they stay finite).

Usage: python profiles/micro/splat_time.py [--reps N] [--n POINTS] [--label TEXT] [--out FILE]
Prints one JSON line and appends it to FILE."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from points_time import emit, make_points, spread  # noqa: E402


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)

    def timed(fn):
        out = []
        for rep in range(args.reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                out.append(a.elapsed_time(b))
        return out

    o, R = fields.config_leaves("256")
    N, n = len(o) * 512, args.n
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, 1.0 / R)
    u = torch.from_numpy(f["vel"]).cuda()
    phi = [torch.from_numpy(f[k]).cuda() for k in ("density", "temperature", "fuel", "waste")]
    gen = torch.Generator(device="cuda").manual_seed(5)
    vals = [torch.randn(n, device="cuda", generator=gen) for _ in phi]
    vvals = torch.randn((n, 3), device="cuda", generator=gen)
    outs = [torch.empty(n, device="cuda") for _ in phi]
    vout = torch.empty((n, 3), device="cuda")
    ordered = make_points(o, n, 9)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)]}
    channel_sets = {
        "1_float": (phi[:1], vals[:1], outs[:1]),
        "velocity": ([u], [vvals], [vout]),
        "4_floats_and_velocity": (phi + [u], vals + [vvals], outs + [vout]),
    }
    line = {"library": os.path.basename(_lib.library_path()), "label": args.label, "reps": args.reps, "log2_quantum": -32,
            "config": f"256: {len(o)} leaves, {N} voxels; {n} points, point values of unit size"}
    for name, pts in sets.items():
        p = torch.from_numpy(pts).cuda()
        res = line[name] = {}
        for label, (dst, src, sampled) in channel_sets.items():
            channels = sum(3 if t.dim() == 2 else 1 for t in dst)
            ts = timed(lambda: device.splat_points(g, dst, p, src))
            tg = timed(lambda: device.sample_points(g, dst, p, sampled))
            res[label] = {"splat_ms": spread(ts), "sample_ms": spread(tg), "splat_ns_per_point_and_channel": round(1e6 * float(np.median(ts)) / (n * channels), 4),
                          "splat_over_sample": round(float(np.median(ts)) / float(np.median(tg)), 3)}
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    device.splat_points(g, phi[:1], p, vals[:1], status=status)
    line["taps_landed_mean"] = round(float(status.float().mean()), 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    emit(measure(args), args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
