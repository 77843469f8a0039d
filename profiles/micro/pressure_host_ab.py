"""Host cost of the pressure loop, two builds of the library alternating in one call (profiles/pressure_host_refactor_ab.txt):
    python profiles/micro/pressure_host_ab.py --parent /path/to/the/other/libhns.so [--reps 5] [--out file.jsonl]
Per repeat and build, each in a fresh process: `python bench.py --gpus 1 --steps 200 --warmup 5` (the default workload, 256^3 with 50 iterations, over a window of 200 substeps), and the launch-bound end -- hns_dev_time_rbgs at 50
iterations on the 8-leaf and the 729-leaf dense grid (`--small`: that child). Stops at the first child that fails or runs into its time limit."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def small():
    sys.path.insert(0, ROOT)
    import torch
    from hnanosolver_amd import _lib, api, device as D, fields

    out = {"library": _lib.library_path()}
    for R, reps in ((16, 2000), (72, 600)):
        o = fields.dense_leaves(R)
        grid = api.create_grid_from_leaves(o, 1.0 / R)
        n = len(o) * 512
        div = torch.randn(n, generator=torch.Generator(device="cpu").manual_seed(R)).cuda()
        p_a, p_b = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        D.time_rbgs(grid, div, p_a, p_b, 1.0 / R, 1.93, 50, 50)  # untimed: code objects, block records
        torch.cuda.synchronize()
        out[f"us_per_solve_{len(o)}_leaves"] = D.time_rbgs(grid, div, p_a, p_b, 1.0 / R, 1.93, 50, reps) * 50 * 1e3  # (it returns the mean ms per iteration)
        out[f"plan_{len(o)}_leaves"] = D.rbgs_plan(grid, 50)[1:]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        return small()
    builds = {"parent": os.path.abspath(args.parent), "branch": os.path.join(ROOT, "hnanosolver_amd", "lib", "libhns.so")}
    jobs = {"bench": ([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "5"], 240), "small": ([sys.executable, os.path.abspath(__file__), "--small"], 120)}
    log = open(args.out, "w") if args.out else None
    for rep in range(args.reps):
        for job, (cmd, limit) in jobs.items():
            for build, lib in builds.items():
                try:
                    r = subprocess.run(cmd, cwd=ROOT, env={**os.environ, "HNS_LIBRARY": lib}, capture_output=True, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    sys.exit(f"{job} {build} repeat {rep}: time limit, stopping")
                if r.returncode != 0:
                    sys.exit(f"{job} {build} repeat {rep}: exit {r.returncode}, stopping\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
                rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                keep = {k: v for k, v in rec.items() if k in ("ms_per_step", "value", "library") or k.startswith(("us_per_solve", "plan_"))}
                line = json.dumps({"repeat": rep, "job": job, "build": build, **keep})
                print(line, flush=True)
                if log:
                    log.write(line + "\n")
                    log.flush()


if __name__ == "__main__":
    main()
