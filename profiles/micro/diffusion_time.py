#!/usr/bin/env python
"""Diffusing a sim (device.Sim.diffuse: hns_diffusion_apply, hns_diffusion.hip) on the dense 256^3 grid, every voxel active, against two yardsticks of the same run,
every form alternating in one process:

  sor2              one blocked SOR launch: hns_dev_rbgs_iterate with two iterations on arrays of the sim's size (12 algorithmic bytes per voxel and iteration: p in,
                    p out, the divergence)
  core_substep      one hns_sim_core_substep with 50 pressure iterations on the sim
  diffuse <terms> <method> [collide]
                    terms: 1 float field, 4 float fields, the velocity, the velocity and 4 fields; method jacobi or chebyshev; with and without a collider (a
                    sphere of a quarter of the extent in collision_sdf). Each form is timed with LOW and with HIGH iterations (both >= 2: no copy launch):
                    per iteration = (t_high - t_low) / (HIGH - LOW); the one-off part (the face launch, the host's work) = t_low - LOW * per iteration.

The byte floor of an iteration: per voxel and float field 12 B (x in, x out, b), 16 for a Chebyshev step (x^(k-2)), the velocity three times that, plus the code bytes
shared between the fields of a launch (1 per voxel, 2 with the velocity); over 8.0 TB/s, the HBM3E peak.

Usage: python profiles/micro/diffusion_time.py [--reps N] [--out FILE]
Prints one JSON line and appends it to FILE (default profiles/diffusion_time_256.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT = 1.0 / 24.0
FLOATS = ["density", "temperature", "fuel", "waste", "flame"]
NAMES = FLOATS + ["collision_sdf"]
LOW, HIGH = 2, 18
PEAK_BYTES_PER_S = 8.0e12
TERMS = {
    "1 field": (["temperature"], False),
    "4 fields": (FLOATS[:4], False),
    "velocity": ([], True),
    "velocity + 4 fields": (FLOATS[:4], True),
}


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def floor_bytes_per_voxel(n_fields, velocity, chebyshev):
    per = 16 if chebyshev else 12
    return per * (n_fields + (3 if velocity else 0)) + (2 if velocity else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--config", default="256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_time_256.jsonl"))
    args = ap.parse_args()

    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)
    o, R = fields.config_leaves(args.config)
    vs, N = 1.0 / R, len(o) * 512
    g = api.create_grid_from_leaves(o, vs)
    sim = device.Sim(g, NAMES)
    f = fields.synthetic_fields(o, R)
    c = g.coords().astype(np.float32)
    sdf = (np.sqrt(((c - R / 2) ** 2).sum(1)) - R / 4).astype(np.float32)  # in voxels: a sphere of a quarter of the extent, solid below 0
    del c
    sim.upload({"vel": f["vel"], **{k: f[k] for k in FLOATS}, "collision_sdf": sdf})
    div, p_a, p_b = (torch.from_numpy(f["density"]).cuda(), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # a = coefficient * DT / vs^2 = 0.5: the time does not depend on it
    coefficient = 0.5 * vs * vs / DT
    forms = {"sor2": lambda: device.rbgs_iterate(g, div, p_a, p_b, vs, 1.9, 2), "core_substep": lambda: sim.core_substep(50, DT, vs, device.current_stream())}
    for terms, (names, velocity) in TERMS.items():
        for method in ("jacobi", "chebyshev"):
            for collide in (False, True):
                for k in (LOW, HIGH):
                    name = f"diffuse {terms} {method}" + (" collide" if collide else "") + f" k{k}"
                    forms[name] = (lambda nm, v, m, cl, it: lambda: sim.diffuse(DT, vs, {x: coefficient for x in nm}, viscosity=coefficient if v else 0.0, iterations=it,
                                                                                method=m, collide=cl, threshold=0.0))(names, velocity, method, collide, k)
    t = {k: [] for k in forms}
    for rep in range(args.reps + 2):  # two warm rounds: code objects, the pool's blocks, the SOR block records
        for k, fn in forms.items():
            ms = once(fn)
            if rep >= 2:
                t[k].append(ms)
    sor_iteration = float(np.median(t["sor2"])) / 2
    line = {"library": os.path.basename(_lib.library_path()), "reps": args.reps, "low": LOW, "high": HIGH, "peak_bytes_per_s": PEAK_BYTES_PER_S,
            "config": f"{args.config}: {len(o)} leaves, {N} voxels, every voxel active; synthetic fields; collider: a sphere of radius {R // 4} voxels", "ms": {}, "diffuse": {}}
    for k in ("sor2", "core_substep"):
        line["ms"][k] = spread(t[k])
    line["sor_ms_per_iteration"] = round(sor_iteration, 4)
    for terms, (names, velocity) in TERMS.items():
        for method in ("jacobi", "chebyshev"):
            for collide in (False, True):
                base = f"diffuse {terms} {method}" + (" collide" if collide else "")
                lo, hi = float(np.median(t[base + f" k{LOW}"])), float(np.median(t[base + f" k{HIGH}"]))
                per = (hi - lo) / (HIGH - LOW)
                floor_ms = floor_bytes_per_voxel(len(names), velocity, method == "chebyshev") * N / PEAK_BYTES_PER_S * 1e3
                units = len(names) + (3 if velocity else 0)  # scalar arrays swept: the SOR yardstick sweeps one
                line["diffuse"][base[8:]] = {"ms_low": spread(t[base + f" k{LOW}"]), "ms_high": spread(t[base + f" k{HIGH}"]), "ms_per_iteration": round(per, 4),
                                             "ms_one_off": round(lo - LOW * per, 4), "floor_ms_per_iteration": round(floor_ms, 4), "over_floor": round(per / floor_ms, 2),
                                             "over_sor_iteration": round(per / sor_iteration, 2), "over_sor_iteration_per_array": round(per / sor_iteration / units, 2)}
    sim.close()
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
