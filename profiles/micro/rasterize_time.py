#!/usr/bin/env python3
"""Points rasterised into fields under a spec (hns_splat_spec: k_splat_radial of hns_rasterize.hip, the weight channel and the average finish of hns_splat.hip) on the set-up
of profiles/micro/splat_time.py: the dense 256^3 grid, n = 2^22 points at random offsets inside the domain, (a) in leaf order and (b) the same points permuted.

For the trilinear cell and for r = 1, 2 and 4 voxels, as a sum and as an average, into one float field and into the velocity: the median of --reps calls, each bracketed
by hipEvents on the launch stream, with min and max beside it, and the adds per second -- landed (point, voxel) pairs times the channels of the accumulator the call
writes (the weight channel of an average included), over the median. The landed pairs are counted by the call itself: a sum of NaN values rejects every landed term and
d_rejected counts them. Terms that round to zero issue no add and are not taken out of the count. Beside every figure stands the existing call, the trilinear sum of the
same values at the same points, measured in the same process.

The question: do adds that are contiguous within a wave instruction (a z-run of a footprint on adjacent lanes) exceed the 22-30 G adds/s the trilinear splat is bound by?

Usage: python profiles/micro/rasterize_time.py [--reps N] [--n POINTS] [--label TEXT] [--out FILE]
Prints one JSON line and appends it to FILE."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from points_time import emit, make_points, spread  # noqa: E402

KERNELS = (("trilinear", None), ("radial", 1.0), ("radial", 2.0), ("radial", 4.0))


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
    u, phi = torch.from_numpy(f["vel"]).cuda(), torch.from_numpy(f["density"]).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    vals, vvals = torch.randn(n, device="cuda", generator=gen), torch.randn((n, 3), device="cuda", generator=gen)
    nans = torch.full((n,), float("nan"), device="cuda")
    ordered = make_points(o, n, 9)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)]}
    targets = {"1_float": ([phi], [vals], 1), "velocity": ([u], [vvals], 3)}
    line = {"library": os.path.basename(_lib.library_path()), "label": args.label, "reps": args.reps, "log2_quantum": -32,
            "config": f"256: {len(o)} leaves, {N} voxels; {n} points, point values of unit size"}
    for name, pts in sets.items():
        p = torch.from_numpy(pts).cuda()
        res = line[name] = {}
        for kernel, radius in KERNELS:
            spec = dict(kernel=kernel, radius=radius)
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            device.splat_points(g, [phi], p, [nans], rejected=count, **spec)
            landed = int(count.cpu()[0])
            row = res[kernel if radius is None else f"radial_r{radius:g}"] = {"landed_voxels_per_point": round(landed / n, 3)}
            for label, (dst, src, channels) in targets.items():
                base = timed(lambda: device.splat_points(g, dst, p, src))
                for mode in ("add", "average"):
                    ts = timed(lambda: device.splat_points(g, dst, p, src, mode=mode, **spec))
                    adds = landed * (channels + (1 if mode == "average" else 0))
                    row[f"{label}_{mode}"] = {"ms": spread(ts), "adds": adds, "g_adds_per_s": round(adds / (float(np.median(ts)) * 1e6), 2),
                                              "trilinear_add_ms_same_run": spread(base)}
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
