#!/usr/bin/env python3
"""Device time of the flux-field pass (deff_flux_field_D: k_flux + k_flux_sections, the call's own hipEvent pair) against the
field adjoint's pass (deff_field_vjp_D: k_vjp + k_pass_final) on the same context, shape and D plane, in the same process.
Both move 32 B per cell (the flux field reads x, D and writes fx, fy; the adjoint's pass reads x, lambda, D and writes g), so
the adjoint's pass is the yardstick: reported are the SLOWEST flux-field run against the FASTEST adjoint run.  Run on the GPU box.

  python tools/measure_flux.py [--runs 5] [--out profiles/flux_results.json]

Two shapes: one 4096 x 4096 image and a stack of 16 images of 1024 x 1024.  Per shape `runs` fresh contexts, each with a
synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field and a random lambda (the passes cost the
same on any field), D = the image's two diffusivities as a plane; per context one call of each pass is dropped, then one call
of each is timed, the flux field first: the two alternate."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402
from effectivediffusivityfvm_amd._capi import check  # noqa: E402

BYTES = 32.0
COPY_STREAM = 4.7e12                                   # B/s: a plain copy stream as measured


def measure(n, nimg, runs):
    cells = n * n * nimg
    rng = np.random.default_rng(1)
    lam = rng.standard_normal((nimg * n, n))
    flux, vjp, plan = [], [], {}
    for _ in range(runs):
        with pkg.Solver(n, n, nimg=nimg) as s:
            s.synth_image(12345, 0)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            D = np.where(s.get_image() > 127, 1e-3, 1.0)
            s.set_adjoint(lam)
            dp = D.ctypes.data_as(C.c_void_p)
            e = (C.c_double * nimg)()
            ms = C.c_float()
            for timed in (False, True):                # no map to the host: the device passes alone
                check(s._L.deff_flux_field_D(s._ctx, dp, 0.0, 1.0, None, None, None, None, C.byref(ms)))
                if timed:
                    flux.append(ms.value)
                check(s._L.deff_field_vjp_D(s._ctx, dp, 0.0, 1.0, None, e, C.byref(ms)))
                if timed:
                    vjp.append(ms.value)
            plan = {k: s.plan_value(k) for k in ("flux_kt", "flux_items", "vjp_kt", "vjp_items")}
    slow, fast = max(flux) * 1e-3, min(flux) * 1e-3
    v_slow, v_fast = max(vjp) * 1e-3, min(vjp) * 1e-3
    return {"mesh": [n, n], "images": nimg, "runs": runs, "plan": plan, "flux_ms": flux, "vjp_ms": vjp,
            "flux_slowest_us": slow * 1e6, "flux_fastest_us": fast * 1e6, "vjp_slowest_us": v_slow * 1e6, "vjp_fastest_us": v_fast * 1e6,
            "flux_slowest_over_vjp_fastest": slow / v_fast, "flux_fastest_over_vjp_fastest": fast / v_fast,
            "model_us_at_copy_stream": cells * BYTES / COPY_STREAM * 1e6,
            "tb_per_s_slowest": cells * BYTES / slow / 1e12, "tb_per_s_fastest": cells * BYTES / fast / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_results.json"), help="'' writes no file")
    a = ap.parse_args()
    out = {"img4096": measure(4096, 1, a.runs), "stack16x1024": measure(1024, 16, a.runs)}
    print(json.dumps({k: {q: v for q, v in r.items() if not q.endswith("_ms")} for k, r in out.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
