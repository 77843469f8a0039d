#!/usr/bin/env python3
"""Sorting points into leaf order (device.PointOrder: hns_point_order_*, hns_pointorder.hip) on the dense 256^3 grid, and what the order is worth to the point calls.

Point sets of n = 2^22: (a) leaf_order -- point p lies in leaf p * leaves / n, as profiles/micro/points_time.py makes them --, (b) permuted -- the same points in random
order --, (c) ball -- an emitter ball of radius 3 voxels on a leaf corner: eight leaves, most lanes of a wave on one key.

Sort: the time of one sort at both levels for each set, and of gather and scatter of 12-byte rows, each the median of --reps calls bracketed by hipEvents on the launch
stream, min and max beside it. The floor a sort is set against is the bytes its launches must move -- per point 12 read and 4 written by the key kernel, 4 read by the
histogram of every pass but the first, 8 read (4 in the first pass) and 8 written by every scatter -- over the 6.29 TB/s a float4 copy reaches on this chip.

Payoff, in one process, the two forms alternating rep by rep: the call on the PERMUTED points (the comparator: every call is unchanged by the sort) against
sort + gather of the positions (and values) + the call on the gathered points + scatter of the results back, for an RK4 trace of 8 steps, a sample of four floats and the
velocity, and a trilinear splat of one float. The break-even number of RK4 steps is the fixed cost (sort, gather, scatter) over what a step saves.

rocPRIM yardstick: with --rocprim PROGRAM (profiles/micro/point_order_rocprim.hip, built on its own, never linked into the library) the unsorted voxel keys of the
permuted set go to a file and the program sorts them, as (key, index) pairs over the same key bits, in a child process once this process is done with the GPU.

Usage: python profiles/micro/point_order_time.py [--reps N] [--n POINTS] [--out FILE] [--ab FILE] [--rocprim PROGRAM] [--keys FILE]
Prints one JSON line and appends it to FILE; writes the short table to the --ab file."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT = 1.0 / 24.0
COPY_TBS = 6.29  # float4 copy, measured


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def med(xs):
    return float(np.median(xs))


def floor_bytes_per_point(passes):
    return 12 + 4 + sum((4 if p else 0) + (8 if p else 4) + 8 for p in range(passes))


def measure(args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def timed(fn, before=None):
        out = []
        for rep in range(args.reps + 3):
            if before:
                before()
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                out.append(a.elapsed_time(b))
        return out

    def alternating(forms, before=None):
        """{name: fn} -> {name: [ms]}: the forms in turn within every rep"""
        out = {k: [] for k in forms}
        for rep in range(args.reps + 3):
            for k, fn in forms.items():
                if before:
                    before()
                a, b = ev(), ev()
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 3:
                    out[k].append(a.elapsed_time(b))
        return out

    o, R = fields.config_leaves("256")
    L, n = len(o), args.n
    vs, inv_dx, N = 1.0 / R, float(R), len(o) * 512
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, vs)
    u = torch.from_numpy(f["vel"]).cuda()
    phi = [torch.from_numpy(f[k]).cuda() for k in ("density", "temperature", "fuel", "waste")]
    rng = np.random.default_rng(9)
    leaf = (np.arange(n, dtype=np.int64) * L) // n
    ordered = (o[leaf].astype(np.float64) + rng.uniform(0.0, 8.0, (n, 3))).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d *= (3.0 * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    ball = (o[L // 2].astype(np.float64) + 8.0 + d).astype(np.float32)
    sets = {"leaf_order": ordered, "permuted": ordered[np.random.default_rng(10).permutation(n)], "ball": ball}
    passes = {lv: max(1, -(-(512 * (L + 1) if lv else L + 1).bit_length() // 8)) for lv in (0, 1)}
    line = {"library": os.path.basename(_lib.library_path()), "reps": args.reps, "config": f"256: {L} leaves, {N} voxels; {n} points", "passes": {"leaf": passes[0], "voxel": passes[1]},
            "floor_bytes_per_point": {"leaf": floor_bytes_per_point(passes[0]), "voxel": floor_bytes_per_point(passes[1])}, "copy_TB_per_s": COPY_TBS}
    po = device.PointOrder(g, n)
    dev = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    for name, x in dev.items():
        res = line[name] = {}
        for lv, level in ((0, "leaf"), (1, "voxel")):
            t = timed(lambda: po.sort(x, level))
            floor_ms = floor_bytes_per_point(passes[lv]) * n / (COPY_TBS * 1e12) * 1e3
            res[f"sort_{level}"] = {"ms": spread(t), "ns_per_point": round(1e6 * med(t) / n, 4), "floor_ms": round(floor_ms, 4), "floor_over_measured": round(floor_ms / med(t), 4)}
        # (the object holds the voxel order of x here)
        rows, out = x, torch.empty_like(x)
        t = timed(lambda: po.gather(rows, out))
        res["gather_12B"] = {"ms": spread(t), "GB_per_s": round((12 + 12 + 4) * n / med(t) / 1e6, 1)}
        t = timed(lambda: po.scatter(rows, out))
        res["scatter_12B"] = {"ms": spread(t), "GB_per_s": round((12 + 12 + 4) * n / med(t) / 1e6, 1)}
    # ---- payoff on the permuted points ----
    x = dev["permuted"]
    xs, work, back = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    pay = line["payoff_on_permuted"] = {}

    def trace_plain(steps):
        device.trace_points(g, u, work, DT, inv_dx, 4, steps, status)

    def trace_sorted(steps):
        po.sort(work, "voxel")
        po.gather(work, xs)
        device.trace_points(g, u, xs, DT, inv_dx, 4, steps, status)
        po.scatter(xs, back)

    for steps in (1, 8):
        t = alternating({"plain": lambda: trace_plain(steps), "sorted": lambda: trace_sorted(steps)}, before=lambda: work.copy_(x))
        pay[f"trace_rk4_{steps}_steps"] = {"plain_ms": spread(t["plain"]), "sort_gather_call_scatter_ms": spread(t["sorted"])}
    po.sort(x, "voxel")
    po.gather(x, xs)
    t = alternating({"permuted": lambda: device.trace_points(g, u, work, DT, inv_dx, 4, 1, status), "gathered": lambda: device.trace_points(g, u, back, DT, inv_dx, 4, 1, status)},
                    before=lambda: (work.copy_(x), back.copy_(xs)))
    step_permuted, step_gathered = med(t["permuted"]), med(t["gathered"])
    fixed = alternating({"sort_gather_scatter": lambda: (po.sort(x, "voxel"), po.gather(x, xs), po.scatter(xs, back))})["sort_gather_scatter"]
    pay["rk4_step_ms"] = {"permuted": round(step_permuted, 4), "gathered": round(step_gathered, 4)}
    pay["sort_gather_scatter_ms"] = spread(fixed)
    pay["break_even_rk4_steps"] = round(med(fixed) / max(step_permuted - step_gathered, 1e-9), 2)
    outs = [torch.empty(n, device="cuda") for _ in range(4)] + [torch.empty((n, 3), device="cuda")]
    outs2 = [torch.empty_like(t_) for t_ in outs]

    def sample_sorted():
        po.sort(x, "voxel")
        po.gather(x, xs)
        device.sample_points(g, phi + [u], xs, outs)
        for a, b in zip(outs, outs2):
            po.scatter(a, b)

    t = alternating({"plain": lambda: device.sample_points(g, phi + [u], x, outs2), "sorted": sample_sorted})
    pay["sample_4_floats_and_velocity"] = {"plain_ms": spread(t["plain"]), "sort_gather_call_scatter_ms": spread(t["sorted"])}
    vals, vals_s = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    target = torch.zeros(N, device="cuda")

    def splat_sorted():
        po.sort(x, "voxel")
        po.gather(x, xs)
        po.gather(vals, vals_s)
        device.splat_points(g, [target], xs, [vals_s])

    t = alternating({"plain": lambda: device.splat_points(g, [target], x, [vals]), "sorted": splat_sorted})
    pay["splat_1_float"] = {"plain_ms": spread(t["plain"]), "sort_gather_call_ms": spread(t["sorted"])}
    if args.keys:  # the unsorted voxel keys of the permuted set: the sorted keys scattered back
        po.sort(x, "voxel")
        keys = po.scatter(po.keys).cpu().numpy().view(np.uint32)
        os.makedirs(os.path.dirname(os.path.abspath(args.keys)), exist_ok=True)
        keys.tofile(args.keys)
        line["keys_bits"] = int((512 * (L + 1)).bit_length())
    po.close()
    return line


def table(line):
    rows = [f"point order on {line['config']}; {line['reps']} reps, medians in ms (min .. max); passes leaf {line['passes']['leaf']}, voxel {line['passes']['voxel']}", ""]
    for name in ("leaf_order", "permuted", "ball"):
        r = line[name]
        for k in ("sort_leaf", "sort_voxel"):
            m = r[k]["ms"]
            rows.append(f"{name:10s} {k:12s} {m['median']:8.4f} ({m['min']:.4f} .. {m['max']:.4f})  floor {r[k]['floor_ms']:.4f} = {r[k]['floor_over_measured']:.2f} of measured")
        for k in ("gather_12B", "scatter_12B"):
            m = r[k]["ms"]
            rows.append(f"{name:10s} {k:12s} {m['median']:8.4f} ({m['min']:.4f} .. {m['max']:.4f})  {r[k]['GB_per_s']} GB/s")
    rows.append("")
    for k, v in line["payoff_on_permuted"].items():
        rows.append(f"{k}: {json.dumps(v)}")
    if "rocprim" in line:
        rows.append(f"rocprim: {json.dumps(line['rocprim'])}")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--rocprim", default=None)
    ap.add_argument("--keys", default=None)
    args = ap.parse_args()
    if args.rocprim and not args.keys:
        ap.error("--rocprim needs --keys FILE")
    # the measurements run in a child, so that the yardstick's child starts only after this one has left the GPU
    if os.environ.get("HNS_POINT_ORDER_CHILD") != "1":
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env={**os.environ, "HNS_POINT_ORDER_CHILD": "1"}, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode or 1
        line = json.loads(r.stdout.strip().splitlines()[-1])
        if args.rocprim:
            y = subprocess.run([args.rocprim, args.keys, str(line["keys_bits"]), str(args.reps)], capture_output=True, text=True, timeout=120)
            line["rocprim"] = json.loads(y.stdout.strip().splitlines()[-1]) if y.returncode == 0 else {"failed": y.returncode, "stderr": y.stderr[-500:]}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        if args.ab:
            with open(args.ab, "w") as fh:
                fh.write(table(line))
        return 0
    print(json.dumps(measure(args)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
