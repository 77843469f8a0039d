#!/usr/bin/env python3
"""The V-cycle pressure solve (hns_sim_set_solve_method) against the SOR loop at 256^3 on the headline input: 32^3 leaves, synthetic fields, one float field,
voxel size 1/256, dt 1/24 -- after one plain core substep of 50 iterations, so that the divergence is the headline's. One process, hipEvents on the stream the
calls run on:

  cycle time        hns_sim_pressure_solve of 1, 2 and 4 V(2,2) cycles at omega = 1 (8 coarse iterations), uncontrolled
  per level         the same one cycle with max_levels = 1 .. depth: what each further level adds (max_levels = 1 is `coarse_iterations` plain sweeps)
  residual history  max|c| relative to the one at p = 0 after every cycle (a monitored solve, a check per cycle) beside the SOR's (a check every two iterations)
  variants          history and one-cycle time of a few other parameter sets (fewer, better-solved levels; omega above 1), eight cycles each
  time to target    for the SOR's level after 50 iterations, 1e-2 and 1e-3: the first SOR iteration / V-cycle at or below it, and the time of the plain,
                    uncontrolled solve of that many iterations / cycles

Usage: python profiles/micro/multigrid_time.py [--reps N] [--max-iterations M] [--max-cycles C] [--out FILE]; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hnanosolver_amd import api, device, fields  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    fn()
    return round(float(np.median([timed(fn) for _ in range(reps)])), 4)


def first_at_or_below(rel, tol, step):
    hit = np.flatnonzero(rel <= tol)
    return int(step * (hit[0] + 1)) if len(hit) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-iterations", type=int, default=600)
    ap.add_argument("--max-cycles", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    R, ITERS = 256, 50
    vs, dt = 1.0 / R, 1.0 / 24.0
    o = fields.dense_leaves(R)
    f = fields.synthetic_fields(o, R)
    g = api.create_grid_from_leaves(o, vs)
    s = device.Sim(g, ["density"])
    s.upload({"vel": f["vel"], "density": f["density"]})
    s.core_substep(ITERS, dt, vs)
    torch.cuda.synchronize()

    # the SOR loop: its history, and the plain solve's time at 50 iterations
    s.solve_control(0.0, 0.0, 2)
    s.pressure_solve(args.max_iterations, vs)
    rep = s.solve_report()
    sor_rel = rep["history"]["max_abs"].astype(np.float64) / float(rep["initial"]["max_abs"])
    s.solve_control(None)
    sor_at_50 = float(sor_rel[ITERS // 2 - 1])
    sor_50_ms = median_ms(lambda: s.pressure_solve(ITERS, vs), args.reps)

    # the V-cycle: depth, history, times
    s.solve_method()
    levels = s.solve_levels()
    s.solve_control(0.0, 0.0, 1)
    s.pressure_solve(args.max_cycles, vs)
    rep_mg = s.solve_report()
    assert rep_mg["initial"]["max_abs"] == rep["initial"]["max_abs"]
    mg_rel = rep_mg["history"]["max_abs"].astype(np.float64) / float(rep_mg["initial"]["max_abs"])
    s.solve_control(None)
    cycles_ms = {str(k): median_ms(lambda: s.pressure_solve(k, vs), args.reps) for k in (1, 2, 4)}
    by_levels = {}
    for m in range(1, len(levels) + 1):
        s.solve_method(max_levels=m)
        by_levels[str(m)] = median_ms(lambda: s.pressure_solve(1, vs), args.reps)
    s.solve_method()
    variants = {}
    for name, kw in (("max_levels_3_coarse_30", dict(max_levels=3, coarse_iterations=30)), ("max_levels_4_coarse_30", dict(max_levels=4, coarse_iterations=30)),
                     ("omega_1.15", dict(omega=1.15)), ("max_levels_3_coarse_30_omega_1.15", dict(max_levels=3, coarse_iterations=30, omega=1.15))):
        s.solve_method(**kw)
        s.solve_control(0.0, 0.0, 1)
        s.pressure_solve(8, vs)
        r = s.solve_report()
        s.solve_control(None)
        variants[name] = {"relative_per_cycle": [float(f"{x:.4g}") for x in r["history"]["max_abs"].astype(np.float64) / float(r["initial"]["max_abs"])],
                          "one_cycle_ms": median_ms(lambda: s.pressure_solve(1, vs), args.reps)}
    s.solve_method()

    targets = {"sor_after_50": sor_at_50, "1e-2": 1e-2, "1e-3": 1e-3}
    to_target = {}
    for name, tol in targets.items():
        it, cy = first_at_or_below(sor_rel, tol, 2), first_at_or_below(mg_rel, tol, 1)
        row = {"relative_max_abs": tol, "sor_iterations": it, "vcycles": cy}
        if it is not None:
            s.solve_method(None)
            row["sor_ms"] = median_ms(lambda: s.pressure_solve(it, vs), args.reps)
        if cy is not None:
            s.solve_method()
            row["vcycle_ms"] = median_ms(lambda: s.pressure_solve(cy, vs), args.reps)
        to_target[name] = row
    line = {
        "config": f"256^3 dense ({len(o)} leaves), the headline input after one core substep of {ITERS} iterations; voxel size 1/{R}; V(2,2), omega 1, 8 coarse iterations",
        "reps": args.reps,
        "leaves_per_level": levels,
        "sor_50_iterations_ms": sor_50_ms,
        "vcycle_solve_ms_by_cycles": cycles_ms,
        "one_cycle_ms_by_max_levels": by_levels,
        "norm": "max_abs of the Gauss-Seidel correction c, relative to the one at p = 0",
        "initial_max_abs": float(rep["initial"]["max_abs"]),
        "vcycle_relative_per_cycle": [float(f"{x:.4g}") for x in mg_rel],
        "sor_relative_every_10_iterations": [float(f"{x:.4g}") for x in sor_rel[4::5]],
        "variants": variants,
        "time_to_target": to_target,
    }
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    s.close()


if __name__ == "__main__":
    main()
