#!/usr/bin/env python3
"""The diagnostics (hns_sim_stats, hns_dev_residual, the controlled solve) at 256^3 on the headline input: 32^3 leaves, synthetic fields, one float
field, voxel size 1/256, dt 1/24 -- after one plain core substep of 50 iterations, so that the divergence and the pressure are the headline's.
Each figure is bracketed by hipEvents on the stream the calls run on, all in one process:

  residual          hns_dev_residual on the sim's divergence and pressure (k_residual + the fold launch; 8 algorithmic B/voxel)
  stats             hns_sim_stats of the velocity and one float field, active masks asked for (two launches, then the records' copy and the wait: 16 B/voxel)
  gradient          hns_dev_subtract_pressure_gradient (28 B/voxel), the yardstick the residual kernel shares its staging with
  d2d copies        torch copy_ of as many bytes as the residual / the gradient launch move (read + write)
  solve             hns_sim_pressure_solve(50) plain against monitored (check_every 10, both tolerances 0), alternating

and, from one monitored solve with a check every 2 iterations: the iteration at which the residual's max_abs first falls to 1e-2, 1e-3 and 1e-4 of
the one at p = 0, and where 50 iterations get to.

Usage: python profiles/micro/diagnostics_time.py [--reps N] [--max-iterations M] [--out FILE]; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields  # noqa: E402
from hnanosolver_amd._lib import lib  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max-iterations", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    R, ITERS = 256, 50
    vs, dt = 1.0 / R, 1.0 / 24.0
    o = fields.dense_leaves(R)
    N = len(o) * 512
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, vs)
    s = device.Sim(g, ["density"])
    s.upload({"vel": f["vel"], "density": f["density"]})
    s.core_substep(ITERS, dt, vs)
    torch.cuda.synchronize()
    div_ptr, p_ptr = lib.hns_sim_divergence_ptr(s._ptr), lib.hns_sim_pressure_ptr(s._ptr)
    rec = device.stats_buffer(1)
    u = torch.from_numpy(f["vel"]).cuda()
    u_out = torch.empty_like(u)
    p = torch.empty(N, dtype=torch.float32, device="cuda").normal_()
    copies = {"residual": 8 * N, "gradient": 28 * N}  # bytes the launch moves; the copy reads half of them and writes half
    bufs = {k: (torch.empty(b // 8, dtype=torch.float32, device="cuda").normal_(), torch.empty(b // 8, dtype=torch.float32, device="cuda")) for k, b in copies.items()}

    def residual():
        device._raise(lib.hns_dev_residual(g.ptr, div_ptr, p_ptr, vs, None, rec.data_ptr(), 0))

    calls = {
        "residual": residual,
        "stats_velocity_and_one_float": lambda: s.stats(["density"], velocity=True),
        "gradient": lambda: device.subtract_pressure_gradient(g, u, p, u_out, float(R)),
        "d2d_copy_residual_bytes": lambda: bufs["residual"][1].copy_(bufs["residual"][0]),
        "d2d_copy_gradient_bytes": lambda: bufs["gradient"][1].copy_(bufs["gradient"][0]),
    }
    times = {k: [] for k in calls}
    solve = {"plain": [], "monitored": []}
    for rep in range(args.reps + 3):
        for k, fn in calls.items():
            t = timed(fn)
            if rep >= 3:
                times[k].append(t)
        for mode in ("plain", "monitored"):
            if mode == "plain":
                s.solve_control(None)
            else:
                s.solve_control(0.0, 0.0, 10)
            t = timed(lambda: s.pressure_solve(ITERS, vs))
            if rep >= 3:
                solve[mode].append(t)
    # how far does the solve get? one monitored solve on the headline's divergence, a check every two iterations
    s.solve_control(0.0, 0.0, 2)
    s.pressure_solve(args.max_iterations, vs)
    rep = s.solve_report()
    rel = rep["history"]["max_abs"].astype(np.float64) / float(rep["initial"]["max_abs"])
    first = {}
    for tol in (1e-2, 1e-3, 1e-4):
        hit = np.flatnonzero((rel <= tol) & (rep["history"]["nan_count"] == 0))
        first[f"{tol:g}"] = int(2 * (hit[0] + 1)) if len(hit) else None
    s.solve_control(None)
    med = {k: float(np.median(v)) for k, v in times.items()}
    line = {
        "config": f"256^3 dense ({len(o)} leaves), the headline input after one core substep of {ITERS} iterations; voxel size 1/{R}",
        "reps": args.reps,
        "ms": {k: spread(v) for k, v in times.items()},
        "bytes": {"residual": 8 * N, "stats_velocity_and_one_float": 16 * N + 64 * len(o), "gradient": 28 * N},
        "TBps_at_median": {"residual": round(8 * N / med["residual"] / 1e9, 3), "stats_velocity_and_one_float": round((16 * N + 64 * len(o)) / med["stats_velocity_and_one_float"] / 1e9, 3),
                           "gradient": round(28 * N / med["gradient"] / 1e9, 3), "d2d_copy_residual_bytes": round(8 * N / med["d2d_copy_residual_bytes"] / 1e9, 3),
                           "d2d_copy_gradient_bytes": round(28 * N / med["d2d_copy_gradient_bytes"] / 1e9, 3)},
        "pressure_solve_50_ms": {k: spread(v) for k, v in solve.items()},
        "monitored_over_plain_at_median": round(float(np.median(solve["monitored"]) / np.median(solve["plain"])), 4),
        "convergence": {
            "norm": "max_abs of the Gauss-Seidel correction c, relative to the one at p = 0",
            "initial_max_abs": float(rep["initial"]["max_abs"]),
            "relative_after_50_iterations": float(rel[24]) if len(rel) > 24 else None,
            "first_iteration_at_or_below": first,
            "iterations_run": rep["iterations"],
            "relative_at_the_end": float(rel[-1]),
            "relative_every_100_iterations": [round(float(x), 6) for x in rel[49::50]],
        },
    }
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    s.close()


if __name__ == "__main__":
    main()
