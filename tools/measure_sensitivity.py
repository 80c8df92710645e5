#!/usr/bin/env python3
"""Device time of the Deff gradient pass (deff_sensitivity: k_sens + k_pass_final, the call's own hipEvent pair) against its
24 B/cell byte model (x 8, D 8, g 8) at the two rates DESIGN.md section 4 measured on this chip, and against one CG iteration
of the same shape (profiles/cg_results.json).  Run on the GPU box.

  python tools/measure_sensitivity.py [--cases img4096,img8192,stack16x1024,stack1024x128] [--runs 10] [--warmup 3]
                                      [--out profiles/sensitivity_results.json] [--kt-scan 1,2,4,8] [--profile] [--stats-out FILE.csv]

Every case: one context, a synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field (the pass
costs the same on any field), `warmup` calls dropped, then `runs` calls; reported are the SLOWEST and the FASTEST run.
--profile: rocprofv3 --kernel-trace --stats of the 4096^2 case alone, in a child process of its own."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402
from effectivediffusivityfvm_amd._capi import check  # noqa: E402

CASES = {"img4096": (4096, 1), "img8192": (8192, 1), "stack16x1024": (1024, 16), "stack1024x128": (128, 1024)}
CG_KEYS = {"img4096": "bench4096", "stack16x1024": "stack16x1024"}   # the same shapes in profiles/cg_results.json
BYTES_PER_CELL = 24.0
COPY_STREAM, PEAK = 4.7e12, 8.0e12                     # B/s: a plain copy stream as measured, the HBM peak


def cg_iteration_us(case):
    """per_iter_us of the same shape in profiles/cg_results.json (the first figure found), or None."""
    path = os.path.join(ROOT, "profiles", "cg_results.json")
    if case not in CG_KEYS or not os.path.exists(path):
        return None

    def find(o):
        if isinstance(o, dict):
            if "per_iter_us" in o:
                return o["per_iter_us"]
            o = list(o.values())
        if isinstance(o, list):
            for v in o:
                r = find(v)
                if r is not None:
                    return r
        return None
    return find(json.load(open(path)).get(CG_KEYS[case]))


def measure(case, runs, warmup, kt=0):
    n, nimg = CASES[case]
    cells = n * n * nimg
    with pkg.Solver(n, n, nimg=nimg) as s:
        s.set_tuning("sens_kt", kt)
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        e = (C.c_double * nimg)()
        ms = C.c_float()
        times = []
        for r in range(warmup + runs):
            check(s._L.deff_sensitivity(s._ctx, None, e, C.byref(ms)))   # no map to the host: the device pass alone
            if r >= warmup:
                times.append(ms.value)
        plan = {"sens_kt": s.plan_value("sens_kt"), "sens_items": s.plan_value("sens_items")}
    slow, fast = max(times) * 1e-3, min(times) * 1e-3
    out = {"mesh": [n, n], "nimg": nimg, "runs": runs, "ms": times, "plan": plan, "euler_image0": e[0],
           "slowest_us": slow * 1e6, "fastest_us": fast * 1e6,
           "model_us_at_copy_stream": cells * BYTES_PER_CELL / COPY_STREAM * 1e6, "model_us_at_peak": cells * BYTES_PER_CELL / PEAK * 1e6,
           "tb_per_s_slowest": cells * BYTES_PER_CELL / slow / 1e12, "tb_per_s_fastest": cells * BYTES_PER_CELL / fast / 1e12,
           "fraction_of_copy_stream_slowest": cells * BYTES_PER_CELL / slow / COPY_STREAM,
           "fraction_of_copy_stream_fastest": cells * BYTES_PER_CELL / fast / COPY_STREAM}
    cg = cg_iteration_us(case)
    out["cg_iteration_us"] = cg
    out["slowest_over_cg_iteration"] = None if cg is None else slow * 1e6 / cg
    return out


def profile(stats_out):
    import csv
    import glob
    import shutil
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "img4096", "--runs", "5", "--out", ""],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": (p.stderr or p.stdout)[-1500:]}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        if not files:
            return {"error": "no kernel stats written"}
        out = {}
        for k in csv.DictReader(open(files[0])):
            out[k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6,
                                            "average_us": float(k["AverageNs"]) / 1e3, "percent": float(k["Percentage"])}
        if stats_out:
            shutil.copy(files[0], stats_out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="img4096,img8192,stack16x1024,stack1024x128")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_results.json"), help="'' writes no file")
    ap.add_argument("--kt-scan", default="", help="also time every case under these \"sens_kt\" values, e.g. 1,2,4,8")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stats-out", default=None)
    a = ap.parse_args()
    out = {}
    for case in a.cases.split(","):
        if case not in CASES:
            raise SystemExit(f"unknown case {case}")
        out[case] = measure(case, a.runs, a.warmup)
        print(json.dumps({case: out[case]}), flush=True)
        for kt in [int(k) for k in a.kt_scan.split(",") if k]:
            r = measure(case, a.runs, a.warmup, kt)
            out[case].setdefault("kt_scan", {})[str(kt)] = {k: r[k] for k in ("plan", "slowest_us", "fastest_us")}
            print(json.dumps({case: {"sens_kt": kt, **out[case]["kt_scan"][str(kt)]}}), flush=True)
    if a.profile:
        out["profile_img4096"] = profile(a.stats_out)
        print(json.dumps({"profile_img4096": out["profile_img4096"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
