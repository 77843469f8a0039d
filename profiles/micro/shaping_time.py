#!/usr/bin/env python
"""Shaping a sim (device.Sim.shape: hns_shaping_apply, hns_shaping.hip) on the dense 256^3 grid, against two yardsticks of the same run, every form alternating in one
process:

  buoyancy          hns_dev_temperature_buoyancy in place on a velocity array of the sim's size and layout (a torch copy: taking the sim's own velocity pointer would
                    switch its look-ahead off for good): the in-place pointwise kernel that moves the same 24 bytes per voxel -- the byte floor in practice
  core_substep      one hns_sim_core_substep with 50 pressure iterations on the sim, so that a share of a substep can be stated
  shape o<octaves> f<frequency> [control] [decay4]
                    1, 2 and 4 octaves (lacunarity 2, gain 0.5) at frequency 1/16 and 1, with and without the control field "flame", with 0 and with 4 decayed fields
  decay4            the four decays alone (k_shape<false>)

With --ab LIBRARY a second build of the library (another form of k_shape: _lib.py loads it through HNS_LIBRARY) is measured against this one: one octave per call at
each of --ab-frequencies, the two libraries in fresh child processes that alternate, --ab-rounds each; a child prints the median of --reps calls per frequency. --ab-name
says what the other build is.

Usage: python profiles/micro/shaping_time.py [--reps N] [--out FILE] [--ab LIBRARY --ab-name NAME]
Prints one JSON line and appends it to FILE (default profiles/shaping_time_256.jsonl)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
DT = 1.0 / 24.0
NAMES = ["density", "temperature", "fuel", "waste", "flame"]
DECAY4 = {"density": (0.5, 0.0), "temperature": (2.0, 0.25), "fuel": (1.0, 0.0), "waste": (0.25, 0.0)}
AB_FREQUENCIES = (1.0 / 16, 1.0 / 7, 0.25, 0.5, 1.0)


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


def turbulence(octaves, frequency, control):
    return dict(amplitude=0.25, frequency=frequency, octaves=octaves, lacunarity=2.0, gain=0.5, seed=3, offset=(0.5, -0.25, 0.125), control="flame" if control else None,
                control_lo=0.0, control_hi=1.0)


def setup():
    import torch

    sys.path.insert(0, ROOT)
    from hnanosolver_amd import _lib, api, device, fields

    torch.cuda.set_device(0)
    o, R = fields.config_leaves("256")
    g = api.create_grid_from_leaves(o, 1.0 / R)
    sim = device.Sim(g, NAMES)
    f = fields.synthetic_fields(o, R)
    sim.upload({"vel": f["vel"], **{k: f[k] for k in NAMES}})
    return torch, _lib, api, device, g, sim, f, o, R


def timer(torch):
    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    return once


def alternating(once, forms, reps, warm=2):
    out = {k: [] for k in forms}
    for rep in range(reps + warm):
        for k, fn in forms.items():
            t = once(fn)
            if rep >= warm:
                out[k].append(t)
    return out


def measure(args):
    torch, _lib, api, device, g, sim, f, o, R = setup()
    lib = _lib.load_library()
    once = timer(torch)
    vs, N = 1.0 / R, len(o) * 512
    vel, temp = torch.from_numpy(f["vel"]).cuda(), torch.from_numpy(f["temperature"]).cuda()

    def buoyancy():
        api._raise(lib.hns_dev_temperature_buoyancy(vel.data_ptr(), temp.data_ptr(), vel.data_ptr(), DT, 0.0, 0.01, N, device.current_stream()))

    forms = {"buoyancy": buoyancy, "core_substep": lambda: sim.core_substep(50, DT, vs, device.current_stream()), "decay4": lambda: sim.shape(DT, None, DECAY4)}
    for octaves in (1, 2, 4):
        for frequency, word in ((1.0 / 16, "1/16"), (1.0, "1")):
            for control in (False, True):
                for decay in (None, DECAY4):
                    name = f"shape o{octaves} f{word}" + (" control" if control else "") + (" decay4" if decay else "")
                    forms[name] = (lambda t, d: lambda: sim.shape(DT, t, d))(turbulence(octaves, frequency, control), decay)
    t = alternating(once, forms, args.reps)
    floor, step = float(np.median(t["buoyancy"])), float(np.median(t["core_substep"]))
    line = {"library": os.path.basename(_lib.library_path()), "reps": args.reps, "dt": DT, "decay4": DECAY4,
            "config": f"256: {len(o)} leaves, {N} voxels, voxel size 1/{R}; synthetic fields; fields {NAMES}", "ms": {}}
    for k, v in t.items():
        row = {"ms": spread(v)}
        if k not in ("buoyancy", "core_substep"):
            row["over_buoyancy"] = round(float(np.median(v)) / floor, 3)
            row["share_of_core_substep"] = round(float(np.median(v)) / step, 4)
        line["ms"][k] = row
    sim.close()
    return line


def child(args):
    """the --ab child: one octave per call at every frequency, median of --reps, as one JSON line"""
    torch, _lib, api, device, g, sim, f, o, R = setup()
    once = timer(torch)
    forms = {f"{fr:.6g}": (lambda t: lambda: sim.shape(DT, t, None))(turbulence(1, fr, False)) for fr in args.ab_frequencies}
    t = alternating(once, forms, args.reps)
    sim.close()
    print("AB " + json.dumps({k: float(np.median(v)) for k, v in t.items()}), flush=True)
    return 0


def ab(args):
    here = os.path.abspath(__file__)
    runs = {"this": [], "other": []}
    for _ in range(args.ab_rounds):
        for which, library in (("this", None), ("other", os.path.abspath(args.ab))):
            env = dict(os.environ)
            env.pop("HNS_LIBRARY", None)
            if library:
                env["HNS_LIBRARY"] = library
            r = subprocess.run([sys.executable, here, "--child", "--reps", str(args.reps), "--ab-frequencies", *[repr(x) for x in args.ab_frequencies]], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"the {which} child failed ({r.returncode}): {r.stdout[-500:]} {r.stderr[-1500:]}")
            runs[which].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {}
    for fr in runs["this"][0]:
        b, t = [x[fr] for x in runs["this"]], [x[fr] for x in runs["other"]]
        out[fr] = {"this_ms": spread(b), "other_ms": spread(t), "other_over_this": round(float(np.median(t)) / float(np.median(b)), 3)}
    return {"other": args.ab_name, "rounds": args.ab_rounds, "one octave per call, median of reps per child; frequency": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shaping_time_256.jsonl"))
    ap.add_argument("--ab", default=None, help="another build of libhns.so to measure against this one")
    ap.add_argument("--ab-name", default="another build")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-frequencies", type=float, nargs="+", default=list(AB_FREQUENCIES))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    line = measure(args)
    if args.ab:
        line["against_another_build"] = ab(args)
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
