#!/usr/bin/env python3
"""Time per iteration of the volume form of conjugate gradients (deff_volume_solve_cg: k_cgv_dir + k_cgp_update and the two
reductions) against the 2-D plane form (deff_solve_cg under "cg_planes" 1) at the same cell count and on the same D values, in
one process.  Reported per pair of shapes: deff_cg_result.loop_ms / iters of the SLOWEST volume run over the FASTEST plane run.
Run on the GPU box.

  python tools/measure_volume.py [--runs 5] [--iters 200] [--out profiles/volume_results.json]

Pairs: 256^3 against 4096^2 (16.8 M cells) and 128^3 against 2048 x 1024.  D is seeded, uniform in [0.5, 2] per cell (no row
dictionary exists for it); the volume's values reshaped are the image's.  Per pair `runs` fresh contexts of each form; on each
one call is dropped and one timed, the volume first: the two alternate.  A call is `iters` iterations from the linear guess
(rtol 0, so that nothing stops it earlier).
Byte model per cell and iteration: the plane form moves 136 B; the volume form adds aB and aF (16 B): 152 B if r, inv and p of
the back and front rows come from cache, up to 200 B if they come from HBM -- a ratio between 1.12 and 1.47.
Also recorded: the iterations of a seeded two-phase 128^3 volume (Ds 1e-3, Df 1, half of the cells each) to rtol 1e-10."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402

CL, CR = 0.0, 1.0
BYTES_2D, BYTES_3D_CACHE, BYTES_3D_HBM = 136.0, 152.0, 200.0


def pair(n3, nx2, ny2, runs, iters):
    assert n3 ** 3 == nx2 * ny2
    cells = n3 ** 3
    D = np.random.default_rng(n3).uniform(0.5, 2.0, (n3, n3, n3))
    vol, img, plan = [], [], {}
    for _ in range(runs):
        with pkg.Volume(n3, n3, n3) as v, pkg.Solver(nx2, ny2) as s:
            v.assemble_from_D(D, CL, CR)
            s.set_tuning("cg_planes", 1)
            s.assemble_from_D(D.reshape(ny2, nx2), CL, CR)
            for timed in (False, True):
                v.init_linear(CL, CR)
                r3 = v.solve_cg(rtol=0.0, max_iter=iters, fluxes=False)
                s.init_linear(CL, CR)
                r2 = s.solve_cg(rtol=0.0, max_iter=iters, fluxes=False)
                assert r3.iters == iters and r2.iters == iters and v.plan_value("cg_impl") == 5 and s.plan_value("cg_impl") == 3
                if timed:
                    vol.append(r3.loop_ms / r3.iters)
                    img.append(r2.loop_ms / r2.iters)
            plan = {"volume": {k: v.plan_value(k) for k in ("cg_kr", "cg_items")},
                    "image": {k: s.plan_value(k) for k in ("cg_kr", "cg_items")}}
    slow, fast = max(vol), min(img)
    return {"volume": [n3, n3, n3], "image": [nx2, ny2], "cells": cells, "runs": runs, "iters_per_call": iters, "plan": plan,
            "volume_ms_per_iter": vol, "image_ms_per_iter": img,
            "volume_slowest_over_image_fastest": slow / fast, "volume_fastest_over_image_slowest": min(vol) / max(img),
            "model_ratio_cache": BYTES_3D_CACHE / BYTES_2D, "model_ratio_hbm": BYTES_3D_HBM / BYTES_2D,
            "volume_tb_per_s_at_152B_slowest": cells * BYTES_3D_CACHE / (slow * 1e-3) / 1e12,
            "image_tb_per_s_at_136B_fastest": cells * BYTES_2D / (fast * 1e-3) / 1e12}


def two_phase(n3, rtol):
    rng = np.random.default_rng(12345)
    D = np.where(rng.random((n3, n3, n3)) < 0.5, 1e-3, 1.0)
    with pkg.Volume(n3, n3, n3) as v:
        v.assemble_from_D(D, CL, CR)
        v.init_linear(CL, CR)
        r = v.solve_cg(rtol=rtol, max_iter=200_000, fluxes=False)
        return {"volume": [n3, n3, n3], "Ds": 1e-3, "Df": 1.0, "rtol": rtol, "iters": r.iters, "converged": r.converged,
                "rel_residual": r.rel_residual, "deff_raw": r.deff_raw, "loop_ms": r.loop_ms,
                "restarts": v.plan_value("cg_restarts")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_results.json"), help="'' writes no file")
    ap.add_argument("--bench-parent", type=float, nargs="*", default=[], help="bench.py's primary row (Mcells*iter/s) with the "
                    "parent's library (DEFF_AMD_LIB) in the same visit: recorded beside the results, nothing is run for it")
    ap.add_argument("--bench-tree", type=float, nargs="*", default=[], help="... and with this tree's")
    a = ap.parse_args()
    out = {"vol256_img4096": pair(256, 4096, 4096, a.runs, a.iters), "vol128_img2048x1024": pair(128, 2048, 1024, a.runs, a.iters),
           "two_phase_128": two_phase(128, 1e-10)}
    if a.bench_parent or a.bench_tree:
        out["bench_primary_row_mcells_iter_per_s"] = {"parent_library": a.bench_parent, "this_tree": a.bench_tree}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
