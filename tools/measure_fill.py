#!/usr/bin/env python3
"""3-phase assembly: the explicit path (host flood fill, deff_assemble_3phase, harvested dictionary) against the native one
(deff_assemble_3phase_native) on the GPU box -> profiles/fill_results.json.

Every step runs in a child process of its own under a time limit; a step that fails or runs out of time ends the run.
  setup   set_image .. ready to sweep (deff_sweeps(ctx, 1) ends both paths, so the old one includes the dictionary harvest),
          fresh contexts, the two paths alternating, RUNS each; the old path's host flood fill is timed separately
  stage   the re-assembly of a continuation stage (another Dg on the same image) up to the first sweep
  fill    the first native assembly of a 4096^2 image alone: launches, most rounds of a workgroup, wall time of the call
  driver  deff2d on N three-level JPEGs of 128^2, RunBatch 1, 3 phases, --fill host and --fill device alternating
usage: measure_fill.py [--images N] [--runs R] [--out file]      (or, internally, --step NAME)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
DS, DF, CL, CR = 0.0, 1.0, 0.0, 1.0


def grains(rng, H, W, nimg=1):
    f = np.kron(rng.random((nimg * H // 8 + 1, W // 8 + 1)), np.ones((8, 8)))[:nimg * H, :W]
    return np.where(f < 0.3, 0, np.where(f < 0.65, 150, 255)).astype(np.uint8)


def spread(v):
    return {"min": min(v), "max": max(v), "runs": len(v)}


def shapes():
    import effectivediffusivityfvm_amd as pkg
    rng = np.random.default_rng(1)
    out = {"128x128": (grains(rng, 128, 128), 1), "256x128x128": (grains(rng, 128, 128, 256), 256),
           "1024x1024": (grains(rng, 1024, 1024), 1), "4096x4096": (grains(rng, 4096, 4096), 1)}
    p42 = os.path.join(ROOT, "tests", "golden", "00042.jpg")
    if os.path.exists(p42):
        out["00042.jpg"] = (pkg.load_jpeg_gray(p42), 1)
    return out


def step_setup(runs):
    import torch  # noqa: F401
    import effectivediffusivityfvm_amd as pkg
    res = {}
    for name, (pix, nimg) in shapes().items():
        ny, nx = pix.shape[0] // nimg, pix.shape[1]
        old, new, host, old_stage, new_stage, plan = [], [], [], [], [], {}
        for _ in range(runs):
            t0 = time.perf_counter()
            grid = np.concatenate([pkg.flood_fill((pix[k * ny:(k + 1) * ny] > 200).astype(np.uint32))[0] for k in range(nimg)])
            host.append((time.perf_counter() - t0) * 1e3)
            for path in ("old", "new"):
                with pkg.Solver(nx, ny, nimg=nimg) as s:
                    s.init_linear(CL, CR)
                    s.synchronize()
                    t0 = time.perf_counter()
                    s.set_image(pix)
                    if path == "old":
                        s.assemble_3phase(DS, DF, 10.0, CL, CR, grid=grid)
                    else:
                        s.assemble_3phase_native(DS, DF, 10.0, CL, CR)
                    s.sweeps(1)
                    s.synchronize()
                    (old if path == "old" else new).append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    if path == "old":
                        s.assemble_3phase(DS, DF, 100.0, CL, CR, grid=grid)
                    else:
                        s.assemble_3phase_native(DS, DF, 100.0, CL, CR)
                    s.sweeps(1)
                    s.synchronize()
                    (old_stage if path == "old" else new_stage).append((time.perf_counter() - t0) * 1e3)
                    if path == "new":
                        plan = {k: s.plan_value(k) for k in ("fill_impl", "fill_launches", "fill_rounds", "fill_fallbacks")}
                        plan["kernel"] = s.kernel_in_use()
        res[name] = {"cells": int(nx) * int(ny) * nimg, "host_flood_fill_ms": spread(host),
                     "setup_ms": {"explicit": spread(old), "native": spread(new),
                                  "slowest_native_over_fastest_explicit": max(new) / min(old),
                                  "slowest_native_over_fastest_explicit_with_host_fill": max(new) / (min(old) + min(host))},
                     "stage_ms": {"explicit": spread(old_stage), "native": spread(new_stage),
                                  "slowest_native_over_fastest_explicit": max(new_stage) / min(old_stage)},
                     "native_plan": plan}
    return res


def step_fill(runs):
    import torch  # noqa: F401
    import effectivediffusivityfvm_amd as pkg
    pix, _ = shapes()["4096x4096"]
    first, again, plan = [], [], {}
    for _ in range(runs):
        with pkg.Solver(4096, 4096) as s:
            s.set_image(pix)
            s.synchronize()
            t0 = time.perf_counter()
            s.assemble_3phase_native(DS, DF, 10.0, CL, CR)
            s.synchronize()
            first.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            s.assemble_3phase_native(DS, DF, 100.0, CL, CR)
            s.synchronize()
            again.append((time.perf_counter() - t0) * 1e3)
            plan = {k: s.plan_value(k) for k in ("fill_impl", "fill_launches", "fill_rounds", "fill_fallbacks")}
    return {"first_assembly_ms_fill_codes_table": spread(first), "later_assembly_ms_table_only": spread(again), "plan": plan}


def step_driver(runs, images):
    from PIL import Image
    res = {"images": images, "host": [], "device": []}
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(0)
        for k in range(images):
            Image.fromarray(grains(rng, 128, 128)).save(os.path.join(d, f"{k:05d}.jpg"), quality=100)
        open(os.path.join(d, "input.txt"), "w").write(
            "Input File:\nPhases: 3\nDs: 0\nDf: 1\nDg: 1237500\nMeshAmpX: 1\nMeshAmpY: 1\nCR: 1\nCL: 0\nOutputName: out.csv\n"
            f"printCMap: 0\nConvergence: 1e-5\nMaxIter: 2000\nVerbose: 0\nRunBatch: 1\nNumImages: {images}\n")
        rows = {}
        for _ in range(runs):
            for fill in ("host", "device"):
                t0 = time.perf_counter()
                r = subprocess.run([EXE, "input.txt", "--json", f"{fill}.json", "--fill", fill, "--precond-maxiter", "2000"], cwd=d,
                                   capture_output=True, text=True, timeout=600)
                res[fill].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr
                rows[fill] = [{k: v for k, v in x.items() if k != "Time"} for x in json.load(open(os.path.join(d, f"{fill}.json")))["results"]]
        res["same_numbers"] = rows["host"] == rows["device"]
    out = {"images": images, "seconds": {"host": spread(res["host"]), "device": spread(res["device"])},
           "slowest_device_over_fastest_host": max(res["device"]) / min(res["host"]), "same_numbers": res["same_numbers"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_results.json"))
    a = ap.parse_args()
    if a.step:
        r = {"setup": lambda: step_setup(a.runs), "fill": lambda: step_fill(a.runs), "driver": lambda: step_driver(a.runs, a.images)}[a.step]()
        print("RESULT " + json.dumps(r))
        return 0
    out = {"runs_each": a.runs, "options": {"Ds": DS, "Df": DF, "CL": CL, "CR": CR}}
    for step, limit in (("setup", 420), ("fill", 120), ("driver", 600)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--runs", str(a.runs), "--images", str(a.images)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{step}: not finished after {limit} s; stopping", flush=True)
            return 1
        if r.returncode != 0:
            print(f"{step}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        out[step] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(f"{step}: done", flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
