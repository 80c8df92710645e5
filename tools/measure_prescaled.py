#!/usr/bin/env python3
"""The pre-scaled five-FMA sweeps (set_tuning("prescaled", 1)) against the default and the contracted ("fma") arithmetic
(run on the GPU box).  One process, one context per workload; the arms alternate run by run, every run is one deff_sweeps
call from the linear guess, timed by deff_sweeps' own event pair; the first round allocates and warms up and is dropped.

  python tools/measure_prescaled.py [--cases bench4096,img8192,stack16x1024,stack1024x128,profile] [--runs 5]
                                    [--out profiles/prescaled_results.json] [--stats-out profiles/prescaled_kernel_stats.csv]

bench4096      bench.py's workload: synthetic 4096^2 (seed 12345), Ds 1e-3, T = 8
img8192        synthetic 8192^2
stack16x1024   16 synthetic 1024^2 images in one stack context
stack1024x128  1 024 synthetic 128^2 images in one stack context
profile        rocprofv3 --kernel-trace --stats of the pre-scaled arm of bench4096 alone, in a child process of its own

Arms: default (what the planner runs: chained passes at 4096^2), default_one_launch ("tb_chain" 0: the launch form the
pre-scaled kernel has), fma, prescaled.  Reported as the project reports A/B results: the SLOWEST pre-scaled run against the
FASTEST run of each other arm (ratio > 1: pre-scaled wins even so), next to best against best."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402

ARMS = (("default", {"fma": 0, "prescaled": 0, "tb_chain": 1}), ("default_one_launch", {"fma": 0, "prescaled": 0, "tb_chain": 0}),
        ("fma", {"fma": 1, "prescaled": 0, "tb_chain": 1}), ("prescaled", {"fma": 0, "prescaled": 1, "tb_chain": 1}))
WORKLOADS = {"bench4096": (4096, 1, 8008), "img8192": (8192, 1, 2008), "stack16x1024": (1024, 16, 8008), "stack1024x128": (128, 1024, 8008)}


def workload(name, runs, arms=ARMS):
    n, nimg, sweeps = WORKLOADS[name]
    cells = n * n * nimg
    rows = {a: [] for a, _ in arms}
    plans = {}
    with pkg.Solver(n, n, nimg=nimg) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        for r in range(runs + 1):
            for arm, keys in arms:
                for k, v in keys.items():
                    s.set_tuning(k, v)
                s.init_linear(0.0, 1.0)
                ms = s.sweeps(sweeps)
                if r:
                    rows[arm].append(ms)
                plans[arm] = dict(s.plan(), tb_chain=s.plan_value("tb_chain"), kernel=s.kernel_in_use())
    out = {"mesh": [n, n], "nimg": nimg, "sweeps_per_run": sweeps, "runs": runs, "ms": rows, "plans": plans,
           "gcells_per_s_best": {a: cells * sweeps / (min(v) * 1e-3) / 1e9 for a, v in rows.items()}}
    if "prescaled" in rows:
        slow = max(rows["prescaled"])
        out["fastest_other_over_slowest_prescaled"] = {a: min(v) / slow for a, v in rows.items() if a != "prescaled"}
        out["best_other_over_best_prescaled"] = {a: min(v) / min(rows["prescaled"]) for a, v in rows.items() if a != "prescaled"}
    return out


def profile(stats_out):
    import csv
    import glob
    import shutil
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "bench4096", "--runs", "2", "--only-prescaled", "--out", run],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0 or not os.path.exists(run):
            return {"error": (p.stderr or p.stdout)[-1500:]}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        if not files:
            return {"error": "no kernel stats written"}
        out = {"run": json.load(open(run))["bench4096"], "kernels": {}}
        for k in csv.DictReader(open(files[0])):
            out["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6,
                                                       "average_us": float(k["AverageNs"]) / 1e3, "percent": float(k["Percentage"])}
        if stats_out:
            shutil.copy(files[0], stats_out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bench4096,img8192,stack16x1024,stack1024x128,profile")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--only-prescaled", action="store_true")
    a = ap.parse_args()
    out = {}
    for case in a.cases.split(","):
        if case == "profile":
            out[case] = profile(a.stats_out)
        elif case in WORKLOADS:
            out[case] = workload(case, a.runs, ARMS[3:] if a.only_prescaled else ARMS)
        else:
            raise SystemExit(f"unknown case {case}")
        print(json.dumps({case: out[case]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
