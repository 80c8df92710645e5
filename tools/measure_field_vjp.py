#!/usr/bin/env python3
"""Device time of the field adjoint's pass (deff_field_vjp_D: k_vjp + k_pass_final, the call's own hipEvent pair) against the Deff
gradient's pass (deff_sensitivity_D: k_sens + k_pass_final) on the same context, shape and D plane in the same run, scaled by
32 / 24 for the third stream (byte models: x, lambda, D read and g written, 32 B/cell, against 24 B/cell); and one adjoint solve
(deff_solve_adjoint) against one forward deff_solve_cg of the same system at the same rtol: iterations and loop_ms.  Run on
the GPU box.

  python tools/measure_field_vjp.py [--cases img4096,stack16x1024,stack1024x128] [--runs 10] [--warmup 3]
                                    [--solve 2048] [--rtol 1e-10] [--out profiles/field_vjp_results.json]
                                    [--profile] [--stats-out FILE.csv]

Every case: one context, a synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field and a random
lambda (the passes cost the same on any field), D = the image's two diffusivities as a plane; `warmup` calls dropped, then
`runs` calls of each pass, alternating; reported are the SLOWEST and the FASTEST run.
--profile: rocprofv3 --kernel-trace --stats of the 4096^2 case alone, in a child process of its own (asked for when the pass
is more than 1.25 x the scaled gradient pass)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402
from effectivediffusivityfvm_amd._capi import check  # noqa: E402

CASES = {"img4096": (4096, 1), "stack16x1024": (1024, 16), "stack1024x128": (128, 1024)}
VJP_BYTES, SENS_BYTES = 32.0, 24.0
COPY_STREAM, PEAK = 4.7e12, 8.0e12                     # B/s: a plain copy stream as measured, the HBM peak
MARGIN = 1.25


def measure(case, runs, warmup):
    n, nimg = CASES[case]
    cells = n * n * nimg
    rng = np.random.default_rng(1)
    with pkg.Solver(n, n, nimg=nimg) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        D = np.where(s.get_image() > 127, 1e-3, 1.0)
        s.set_adjoint(rng.standard_normal((n * nimg, n)))
        dp = D.ctypes.data_as(C.c_void_p)
        e = (C.c_double * nimg)()
        ms = C.c_float()
        vjp, sens = [], []
        for r in range(warmup + runs):
            check(s._L.deff_field_vjp_D(s._ctx, dp, 0.0, 1.0, None, e, C.byref(ms)))      # no map to the host: the device pass alone
            if r >= warmup:
                vjp.append(ms.value)
            check(s._L.deff_sensitivity_D(s._ctx, dp, 0.0, 1.0, None, e, C.byref(ms)))
            if r >= warmup:
                sens.append(ms.value)
        plan = {k: s.plan_value(k) for k in ("vjp_kt", "vjp_items", "sens_kt", "sens_items")}
    slow, fast = max(vjp) * 1e-3, min(vjp) * 1e-3
    s_slow, s_fast = max(sens) * 1e-3, min(sens) * 1e-3
    scale = VJP_BYTES / SENS_BYTES
    return {"mesh": [n, n], "nimg": nimg, "runs": runs, "plan": plan, "vjp_ms": vjp, "sens_ms": sens,
            "vjp_slowest_us": slow * 1e6, "vjp_fastest_us": fast * 1e6,
            "sens_slowest_us": s_slow * 1e6, "sens_fastest_us": s_fast * 1e6,
            "sens_scaled_slowest_us": s_slow * scale * 1e6, "sens_scaled_fastest_us": s_fast * scale * 1e6,
            "vjp_over_scaled_sens_slowest": slow / (s_slow * scale), "vjp_over_scaled_sens_fastest": fast / (s_fast * scale),
            "within_margin": bool(slow <= MARGIN * s_slow * scale and fast <= MARGIN * s_fast * scale),
            "model_us_at_copy_stream": cells * VJP_BYTES / COPY_STREAM * 1e6, "model_us_at_peak": cells * VJP_BYTES / PEAK * 1e6,
            "tb_per_s_slowest": cells * VJP_BYTES / slow / 1e12, "tb_per_s_fastest": cells * VJP_BYTES / fast / 1e12,
            "fraction_of_copy_stream_slowest": cells * VJP_BYTES / slow / COPY_STREAM,
            "fraction_of_copy_stream_fastest": cells * VJP_BYTES / fast / COPY_STREAM}


def solves(n, rtol):
    """One forward solve_cg on the row table, one on the coefficient planes ("cg_planes" 2: the kernels the adjoint solve
    runs) and one adjoint solve with w = N(0, 1), on the synthetic 2-phase system of an n x n image."""
    rng = np.random.default_rng(2)
    w = rng.standard_normal((n, n))
    out = {"mesh": [n, n], "rtol": rtol}
    with pkg.Solver(n, n) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        for key, planes in (("forward_table", 0), ("forward_planes", 2)):
            s.set_tuning("cg_planes", planes)
            s.init_linear(0.0, 1.0)
            r = s.solve_cg(rtol=rtol, fluxes=False)
            out[key] = {"iters": r.iters, "loop_ms": r.loop_ms, "rel_residual": r.rel_residual, "converged": r.converged,
                        "per_iter_us": r.loop_ms * 1e3 / max(r.iters, 1), "cg_impl": s.plan_value("cg_impl")}
        r = s.solve_adjoint(w, rtol=rtol)
        out["adjoint"] = {"iters": r.iters, "loop_ms": r.loop_ms, "rel_residual": r.rel_residual, "converged": r.converged,
                          "per_iter_us": r.loop_ms * 1e3 / max(r.iters, 1), "cg_impl": s.plan_value("cg_impl")}
    return out


def profile(stats_out):
    import csv
    import glob
    import shutil
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "img4096", "--runs", "5", "--solve", "", "--out", ""],
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
    ap.add_argument("--cases", default="img4096,stack16x1024,stack1024x128")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--solve", default="2048", help="square meshes for the adjoint-against-forward solve, e.g. 2048,4096; '' = none")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_vjp_results.json"), help="'' writes no file")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stats-out", default=None)
    a = ap.parse_args()
    out = {}
    for case in [c for c in a.cases.split(",") if c]:
        if case not in CASES:
            raise SystemExit(f"unknown case {case}")
        out[case] = measure(case, a.runs, a.warmup)
        print(json.dumps({case: {k: v for k, v in out[case].items() if not k.endswith("_ms")}}), flush=True)
    for n in [int(v) for v in a.solve.split(",") if v]:
        out[f"solve{n}"] = solves(n, a.rtol)
        print(json.dumps({f"solve{n}": out[f"solve{n}"]}), flush=True)
    if a.profile:
        out["profile_img4096"] = profile(a.stats_out)
        print(json.dumps({"profile_img4096": out["profile_img4096"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
