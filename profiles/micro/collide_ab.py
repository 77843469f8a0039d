#!/usr/bin/env python3
"""A/B of the substep with a collision SDF: option "collide" = auto (32-bit addressed advection kernels with the SDF in an LDS box, fused divergence + combustion +
buoyancy, q4 advect_scalars) against "collide" = generic (the 64-bit addressed k_advect_vector<true> / k_advect_scalars<true> and three pointwise launches) and, with
--parent, against another build of the library (HNS_LIBRARY: the commit before these kernels). Also the substep WITHOUT a collider, for the ratio (and that of the other build).

256^3 dense-active, S = 5, fields.sphere_sdf collider, 50 pressure iterations, hipEvents around the five stages (hns_sim_stage_timing). A library is chosen when the
process starts, so every leg of every round is a process of its own, one at a time, the legs alternating: 3 rounds x 10 timed substeps per leg. Before anything is
timed every leg runs once untimed and hashes every field after 3 substeps: the legs with a collider must agree with each other, and so must the two without, or nothing is
timed. (Every timed leg hashes again, and the summary says whether all of them agreed.) One JSON line per leg and round, then one summary line.

    python profiles/micro/collide_ab.py [--parent PATH/libhns.so] [--config 256] [--out FILE.jsonl]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
NAMES = ["density", "temperature", "fuel", "waste", "flame", "collision_sdf"]
STAGES = "advect_vector (+ collision, vorticity off) | divergence + combustion + buoyancy | pressure | gradient (+ collision) | advect_scalars S=5"


def leg(args):
    """one leg in this process: {"leg", "digest", "us": {stage: us per substep}, "plan"}"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib

    if args.leg.startswith("parent"):
        _lib.SIGNATURES.pop("hns_sim_substep_plan", None)  # (the older build has no plan query)
    import hnanosolver_amd as H
    from hnanosolver_amd import api, device as D, fields

    coll = not args.leg.endswith("no_collider")
    if args.leg in ("auto", "generic"):
        H.set_option("collide", args.leg)
    origins, R = fields.config_leaves(args.config)
    vs = 1.0 / R
    f = fields.synthetic_fields(origins, R)
    f["collision_sdf"] = fields.sphere_sdf(origins, R)
    grid = api.create_grid_from_leaves(origins, vs)
    sim = D.Sim(grid, NAMES)
    sim.upload({"vel": f["vel"], **{n: f[n] for n in NAMES}})
    prm = api.CombustionParams(vorticityScale=0.0)
    st = D.current_stream()
    plan = " ".join(f"{k}={v}" for k, v in sim.substep_plan(prm, coll).items()) if not args.leg.startswith("parent") else ""
    for _ in range(3):
        sim.substep(50, 1.0 / 24.0, vs, prm, coll, st)
    torch.cuda.synchronize()
    out = {n: np.empty_like(f[n]) for n in NAMES[:-1]}
    out["vel"] = np.empty_like(f["vel"])
    sim.download(out)
    h = hashlib.sha256()
    for n in sorted(out):
        h.update(out[n].tobytes())
    us = {}
    if args.timed:
        sim.stage_timing(args.timed)
        for _ in range(args.timed):
            sim.substep(50, 1.0 / 24.0, vs, prm, coll, st)
        torch.cuda.synchronize()
        ms, n = sim.stage_times()
        us = {k: round(1e3 * v / n, 1) for k, v in ms.items()}
        us["substep"] = round(sum(us.values()), 1)
    sim.close()
    print(json.dumps({"leg": args.leg, "config": args.config, "leaves": len(origins), "digest": h.hexdigest()[:16], "us": us, "plan": plan}), flush=True)


def agree(lines):
    """one digest among the legs with a collider, another one among those without"""
    with_collider = {x["digest"] for x in lines if not x["leg"].endswith("no_collider")}
    without = {x["digest"] for x in lines if x["leg"].endswith("no_collider")}
    return len(with_collider) == 1 and len(without) == 1 and not (without & with_collider)


def main(args):
    legs = ["auto", "generic"] + (["parent"] if args.parent else []) + ["no_collider"] + (["parent_no_collider"] if args.parent else [])

    def run(name, rnd, timed):
        env = dict(os.environ)
        if name.startswith("parent"):
            env["HNS_LIBRARY"] = os.path.abspath(args.parent)
        else:
            env.pop("HNS_LIBRARY", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--config", args.config, "--timed", str(timed)], env=env, capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:  # nothing more is started on the device after a leg that failed
            sys.exit(f"leg {name} round {rnd} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec["round"] = rnd
        print(json.dumps(rec), flush=True)
        return rec

    check = [run(name, "check", 0) for name in legs]
    if not agree(check):
        sys.exit("the legs disagree: nothing is timed")
    lines = [run(name, rnd, args.timed) for rnd in range(args.rounds) for name in legs]
    same = agree(check + lines)
    summary = {"summary": True, "config": args.config, "bit_identical_after_3_substeps": same, "stages": STAGES, "us_min_max": {}}
    for name in legs:
        mine = [x["us"] for x in lines if x["leg"] == name]
        summary["us_min_max"][name] = {k: [min(m[k] for m in mine), max(m[k] for m in mine)] for k in mine[0]}
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for x in check + lines + [summary]:
                fh.write(json.dumps(x) + "\n")
    if not same:
        sys.exit("the legs disagree: no time counts")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["auto", "generic", "parent", "no_collider", "parent_no_collider"])
    ap.add_argument("--parent")
    ap.add_argument("--config", default="256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    leg(a) if a.leg else main(a)
