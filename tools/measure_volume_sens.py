#!/usr/bin/env python3
"""Device time of the Deff gradient of a volume (deff_volume_sensitivity_D: k_sens3 + k_pass_final) against the 2-D pass
(deff_sensitivity_D: k_sens + k_pass_final) at the same cell count and on the same D values, in one process.  Reported per pair
of shapes: the call's own `ms` of the SLOWEST volume call over the FASTEST image call, and fastest over fastest.  Run on the
GPU box.

  python tools/measure_volume_sens.py [--runs 5] [--out profiles/volume_sens_results.json]

Pairs: 256^3 against 4096^2 (16.8 M cells) and 128^3 against 2048 x 1024.  D is seeded, uniform in [0.5, 2] per cell, the field
seeded, uniform in [0, 1]; the volume's values reshaped are the image's.  Per pair `runs` fresh contexts of each form; on each
one call is dropped and one timed, the volume first: the two alternate.
Byte model per cell: the 2-D pass reads x and D and writes g, 24 B; the volume pass moves the same 24 B if x and D of the back
and front rows come from cache, up to 56 B if they come from HBM -- a ratio between 1.0 and 2.33."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402

CL, CR = 0.0, 1.0
BYTES_2D, BYTES_3D_CACHE, BYTES_3D_HBM = 24.0, 24.0, 56.0


def pair(n3, nx2, ny2, runs):
    assert n3 ** 3 == nx2 * ny2
    cells = n3 ** 3
    rng = np.random.default_rng(n3)
    D = rng.uniform(0.5, 2.0, (n3, n3, n3))
    x = rng.uniform(0.0, 1.0, (n3, n3, n3))
    vol, img, plan = [], [], {}
    for _ in range(runs):
        with pkg.Volume(n3, n3, n3) as v, pkg.Solver(nx2, ny2) as s:
            v.set_field(x)
            s.set_field(x.reshape(ny2, nx2))
            for timed in (False, True):
                _, e3, ms3 = v.sensitivity(D, CL, CR, timing=True)
                _, e2, ms2 = s.sensitivity(D.reshape(ny2, nx2), CL, CR, timing=True)
                assert np.isfinite(e3) and np.isfinite(e2)
                if timed:
                    vol.append(ms3)
                    img.append(ms2)
            plan = {"volume": {k: v.plan_value(k) for k in ("sens_kt", "sens_items")},
                    "image": {k: s.plan_value(k) for k in ("sens_kt", "sens_items")}}
    slow, fast = max(vol), min(img)
    return {"volume": [n3, n3, n3], "image": [nx2, ny2], "cells": cells, "runs": runs, "plan": plan,
            "volume_ms": vol, "image_ms": img,
            "volume_slowest_over_image_fastest": slow / fast, "volume_fastest_over_image_fastest": min(vol) / fast,
            "model_ratio_cache": BYTES_3D_CACHE / BYTES_2D, "model_ratio_hbm": BYTES_3D_HBM / BYTES_2D,
            "volume_tb_per_s_at_24B_slowest": cells * BYTES_3D_CACHE / (slow * 1e-3) / 1e12,
            "volume_tb_per_s_at_56B_slowest": cells * BYTES_3D_HBM / (slow * 1e-3) / 1e12,
            "image_tb_per_s_at_24B_fastest": cells * BYTES_2D / (fast * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_sens_results.json"), help="'' writes no file")
    ap.add_argument("--bench-parent", type=float, nargs="*", default=[], help="bench.py's primary row (Mcells*iter/s) with the "
                    "parent's library (DEFF_AMD_LIB) in the same visit: recorded beside the results, nothing is run for it")
    ap.add_argument("--bench-tree", type=float, nargs="*", default=[], help="... and with this tree's")
    a = ap.parse_args()
    out = {"vol256_img4096": pair(256, 4096, 4096, a.runs), "vol128_img2048x1024": pair(128, 2048, 1024, a.runs)}
    if a.bench_parent or a.bench_tree:
        out["bench_primary_row_mcells_iter_per_s"] = {"parent_library": a.bench_parent, "this_tree": a.bench_tree}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
