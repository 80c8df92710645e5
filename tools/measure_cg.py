#!/usr/bin/env python3
"""deff_solve_cg against the Jacobi loop (run on the GPU box): per case the CG iteration count to rtol, the time to rtol
(loop_ms: the whole CG loop, start and true-residual passes included), the device time per iteration, and Deff next to the
Jacobi Deff at the reference's stopping rule (tol 1e-6, checks every 10 000 sweeps).

  python tools/measure_cg.py [--cases config1,config2,bench4096,stack16x1024,shipped00042] [--rtol 1e-10]
                             [--max-iter N] [--no-jacobi] [--out profiles/cg_results.json]

config1       00000.jpg 128^2, Ds 1e-3, Df 1 (Jacobi run here)
config2       synthetic 1024^2 (seed 12345, image 0), Ds 1e-3 (Jacobi run here)
bench4096     bench.py's workload: synthetic 4096^2 (seed 12345), Ds 1e-3 (Jacobi: profiles/r04_iterations_to_tolerance_4096.log,
              47 200 001 sweeps, 610 s -- not rerun)
stack16x1024  16 synthetic 1024^2 images (seed 12345, images 0-15) in one stack context (Jacobi not run: image 0 is config2)
shipped00042  the reference's shipped input.txt on 00042.jpg through `deff2d --solver cg` (Jacobi: profiles/r04_as_shipped_00042.json)
The bytes model of one iteration is 68 B/cell; "model_us" is that traffic at 6.3 TB/s."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import effectivediffusivityfvm_amd as pkg  # noqa: E402

BYTES_PER_CELL = 68
HBM_TBS = 6.3


def cg_row(r, cells):
    per_it_us = 1e3 * r.loop_ms / max(1, r.iters)
    model_us = cells * BYTES_PER_CELL / (HBM_TBS * 1e12) * 1e6
    return {"iters": int(r.iters), "rel_residual": r.rel_residual, "converged": bool(r.converged), "deff_raw": r.deff_raw,
            "loop_ms": r.loop_ms, "per_iter_us": per_it_us, "model_us": model_us, "per_iter_over_model": per_it_us / model_us}


def synth_case(n, nimg, rtol, max_iter, jacobi):
    with pkg.Solver(n, n, nimg=nimg) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        t0 = time.perf_counter()
        rs = s.solve_cg(rtol=rtol, max_iter=max_iter, fluxes=False)
        wall = time.perf_counter() - t0
        rs = rs if isinstance(rs, list) else [rs]
        out = {"mesh": [n, n], "nimg": nimg, "wall_s": wall, "cg": [cg_row(r, n * n * nimg) for r in rs]}
        if jacobi:
            s.init_linear(0.0, 1.0)
            rj = s.solve(1e-6, 50_000_000)
            out["jacobi"] = {"sweeps": rj.iters, "deff_raw": rj.deff_raw, "loop_ms": rj.loop_ms}
    return out


def config1(rtol, max_iter, jacobi):
    pix = np.load(os.path.join(ROOT, "tests", "golden", "img00000_pix_stb.npy"))
    ny, nx = pix.shape
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        r = s.solve_cg(rtol=rtol, max_iter=max_iter)
        out = {"mesh": [nx, ny], "nimg": 1, "cg": [cg_row(r, nx * ny)]}
        if jacobi:
            s.init_linear(0.0, 1.0)
            rj = s.solve(1e-6, 500_000)
            out["jacobi"] = {"sweeps": rj.iters, "deff_raw": rj.deff_raw, "loop_ms": rj.loop_ms}
    return out


def shipped00042(rtol):
    exe = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(ROOT, "tests", "golden", "00042.jpg"), os.path.join(d, "00042.jpg"))
        kv = dict(Phases=3, Ds=0, Df=1, Dg=1237500, MeshAmpX=1, MeshAmpY=1, InputName="00042.jpg", CR=1, CL=0,
                  OutputName="singleTest.csv", printCMap=0, CMapName="CMAP.csv", Convergence="1e-5", MaxIter="5e5",
                  Verbose=0, RunBatch=0, NumImages=500)
        open(os.path.join(d, "input.txt"), "w").write("Input File:\n" + "".join(f"{k}: {v}\n" for k, v in kv.items()))
        t0 = time.perf_counter()
        p = subprocess.run([exe, "--json", "res.json", "--solver", "cg", "--cg-rtol", repr(rtol)], cwd=d, capture_output=True,
                           text=True, timeout=1800)
        wall = time.perf_counter() - t0
        if p.returncode != 0:
            return {"error": p.stderr[-2000:]}
        res = json.load(open(os.path.join(d, "res.json")))["results"][0]
        csv = open(os.path.join(d, "singleTest.csv")).read().splitlines()
    ref = json.load(open(os.path.join(ROOT, "profiles", "r04_as_shipped_00042.json")))
    return {"deff2d_wall_s": wall, "cg": res, "csv": csv, "jacobi_recorded": ref.get("csv"),
            "jacobi_note": "profiles/r04_as_shipped_00042.json: 5 650 001 sweeps in all, final stage 0.984 s"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="config1,config2,bench4096,stack16x1024,shipped00042")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=2_000_000)
    ap.add_argument("--no-jacobi", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    jac = not a.no_jacobi
    out = {"rtol": a.rtol, "bytes_per_cell_model": BYTES_PER_CELL, "hbm_TBs_model": HBM_TBS}
    for case in a.cases.split(","):
        t0 = time.perf_counter()
        if case == "config1":
            out[case] = config1(a.rtol, a.max_iter, jac)
        elif case == "config2":
            out[case] = synth_case(1024, 1, a.rtol, a.max_iter, jac)
        elif case == "bench4096":
            out[case] = synth_case(4096, 1, a.rtol, a.max_iter, False)
            log = os.path.join(ROOT, "profiles", "r04_iterations_to_tolerance_4096.log")
            out[case]["jacobi_recorded"] = json.loads(open(log).read().splitlines()[-1])
        elif case == "stack16x1024":
            out[case] = synth_case(1024, 16, a.rtol, a.max_iter, False)
        elif case == "shipped00042":
            out[case] = shipped00042(a.rtol)
        else:
            raise SystemExit(f"unknown case {case}")
        out[case]["case_wall_s"] = time.perf_counter() - t0
        print(json.dumps({case: out[case]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
