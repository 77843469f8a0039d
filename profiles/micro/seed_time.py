#!/usr/bin/env python3
"""The seeds of a point set on the device (hns_dev_point_leaves, hns_seed.hip) and the seeded regrid (hns_sim_regrid_seeded) on the dense 256^3 grid, n = 2^22 points
in three orders:

  leaf_order  random offsets inside the domain, point p in leaf p * leaves / n (the set of profiles/micro/points_time.py)
  permuted    the same points randomly permuted
  ball        every point within 3 voxels of the centre of the +x face: an emitter astride the face, eight leaves in all

`seed_ms` brackets one hns_dev_point_leaves call in its query form (no output arrays) with hipEvents on the launch stream: the clears of the key table and of the masks,
k_seed_keys, k_seed_compact, the read-back of the leaf count the masks are sized from, and k_seed_masks -- everything the regrid pays for its seeds, nothing that crosses
PCIe but the count. The yardstick beside it, in the same process, is hns_dev_sample_points (k_sample_points) of one float field at the same points: the same cell work
with loads in place of the hash. Each figure is the median of --reps calls with min and max; nothing is gated. The device result is checked once per order against the host
mirror (hns_point_leaves).

Separately: hns_sim_regrid_times of a seeded regrid (the ball, and the leaf-order points) next to an unseeded regrid of the same sim state at padding 1, --regrid-reps
fresh sims each.

Usage: python profiles/micro/seed_time.py [--reps N] [--n POINTS] [--regrid-reps N] [--label TEXT] [--out FILE]
Prints one JSON line and appends it to FILE."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from points_time import emit, make_points, spread  # noqa: E402

NAMES = ["density", "fuel", "waste", "temperature", "flame"]


def ball(centre, n, seed, radius=3.0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return (np.asarray(centre, dtype=np.float64) + d).astype(np.float32)


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields, leafio

    torch.cuda.set_device(0)
    lib = _lib.load_library()

    def timed(fn, reps):
        out = []
        for rep in range(reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                out.append(a.elapsed_time(b))
        return out

    o, R = fields.config_leaves("256")
    n = args.n
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, 1.0 / R)
    phi = torch.from_numpy(f["density"]).cuda()
    sampled = torch.empty(n, device="cuda")
    ordered = make_points(o, n, 9)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)], "ball": ball((R, R / 2, R / 2), n, 11)}
    line = {"library": os.path.basename(_lib.library_path()), "label": args.label, "reps": args.reps, "config": f"256: {len(o)} leaves; {n} points"}
    leaves, skipped = C.c_uint64(0), C.c_uint64(0)
    for name, pts in sets.items():
        p = torch.from_numpy(pts).cuda()
        got, want = device.point_leaves(p), leafio.point_leaves(pts)
        assert all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and got[2] == want[2], name
        st = device.current_stream()
        ts = timed(lambda: api._raise(lib.hns_dev_point_leaves(0, p.data_ptr(), n, None, None, 0, C.byref(leaves), C.byref(skipped), st)), args.reps)
        tg = timed(lambda: device.sample_points(g, [phi], p, [sampled]), args.reps)
        line[name] = {"seed_leaves": int(leaves.value), "seed_ms": spread(ts), "sample_ms": spread(tg), "seed_ns_per_point": round(1e6 * float(np.median(ts)) / n, 4),
                      "seed_over_sample": round(float(np.median(ts)) / float(np.median(tg)), 3)}
    del phi, sampled
    # the regrid with and without seeds, fresh sims of one state
    state = {k: f[k] for k in ["vel"] + NAMES}
    regrids = {"unseeded": None, "seeded_ball": torch.from_numpy(sets["ball"]).cuda(), "seeded_leaf_order": torch.from_numpy(sets["leaf_order"]).cuda()}
    res = line["regrid_times_ms_padding_1"] = {}
    for name, pts in regrids.items():
        runs = []
        for _ in range(args.regrid_reps):
            s = device.Sim(g, NAMES)
            s.upload(state)
            ng = s.regrid(1, points=pts) if pts is not None else s.regrid(1)
            t = s.regrid_times()
            t["new_leaves"] = ng.leaf_count()
            runs.append(t)
            s.close()
        res[name] = {k: round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--regrid-reps", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    emit(measure(args), args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
