#!/usr/bin/env python3
"""Device time of the second-order field adjoint's pass (deff_field_vjp_hvp_D: k_fhvp + k_pass_final, the call's own hipEvent
pair) against the Deff Hessian-vector pass (deff_sensitivity_hvp_D: k_hvp + k_pass_final) on the same context, shape and planes,
interleaved in the same process.  The new pass moves 56 B per cell (six planes read, one map written) at three waves per SIMD,
the Deff pass 40 B at four; both make three divisions per face: the yardstick is the Deff pass's fastest run scaled by 56 / 40.
Reported are the SLOWEST and the FASTEST k_fhvp run against that yardstick, beside the Deff pass's own slowest / fastest spread
in the same run, and the rate at 56 B per cell.  Nothing was promised for this kernel before it was measured: the figures say
where it stands.  Run on the GPU box.

  python tools/measure_field_hvp.py [--n 4096] [--runs 10] [--warmup 3] [--out profiles/field_hvp_results.json]

One context, a synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field, a random lambda, dx and
dlambda through the setters and a random direction (the passes cost the same on any planes), D = the image's two diffusivities
as a plane; `warmup` calls dropped, then `runs` calls of each pass, alternating."""
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

BYTES, BYTES_HVP = 56.0, 40.0
COPY_STREAM = 4.7e12                                   # B/s: a plain copy stream as measured


def measure(n, runs, warmup):
    cells = n * n
    rng = np.random.default_rng(1)
    with pkg.Solver(n, n) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        D = np.where(s.get_image() > 127, 1e-3, 1.0)
        dD = D * rng.standard_normal((n, n))
        s.set_adjoint(rng.standard_normal((n, n)))
        s.set_tangent(rng.standard_normal((n, n)))
        s.set_adjoint_tangent(rng.standard_normal((n, n)))
        dp, ddp = D.ctypes.data_as(C.c_void_p), dD.ctypes.data_as(C.c_void_p)
        e = (C.c_double * 1)()
        ms = C.c_float()
        fhvp, hvp = [], []
        for r in range(warmup + runs):
            check(s._L.deff_field_vjp_hvp_D(s._ctx, dp, ddp, 0.0, 1.0, None, e, C.byref(ms)))     # no map to the host: the device pass alone
            if r >= warmup:
                fhvp.append(ms.value)
            check(s._L.deff_sensitivity_hvp_D(s._ctx, dp, ddp, 0.0, 1.0, None, e, C.byref(ms)))
            if r >= warmup:
                hvp.append(ms.value)
        plan = {k: s.plan_value(k) for k in ("fhvp_kt", "fhvp_items", "hvp_kt", "hvp_items")}
    slow, fast = max(fhvp) * 1e-3, min(fhvp) * 1e-3
    h_slow, h_fast = max(hvp) * 1e-3, min(hvp) * 1e-3
    scale = BYTES / BYTES_HVP
    ratio, spread = slow / (scale * h_fast), h_slow / h_fast
    return {"mesh": [n, n], "runs": runs, "plan": plan, "fhvp_ms": fhvp, "hvp_ms": hvp,
            "fhvp_slowest_us": slow * 1e6, "fhvp_fastest_us": fast * 1e6, "hvp_slowest_us": h_slow * 1e6, "hvp_fastest_us": h_fast * 1e6,
            "yardstick_us": scale * h_fast * 1e6,                  # the Deff pass's fastest run x 56 / 40
            "fhvp_slowest_over_yardstick": ratio, "fhvp_fastest_over_yardstick": fast / (scale * h_fast),
            "hvp_slowest_over_fastest": spread, "within_hvp_spread": bool(ratio <= spread),
            "model_us_at_copy_stream": cells * BYTES / COPY_STREAM * 1e6,
            "tb_per_s_slowest": cells * BYTES / slow / 1e12, "tb_per_s_fastest": cells * BYTES / fast / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_hvp_results.json"), help="'' writes no file")
    a = ap.parse_args()
    out = {f"img{a.n}": measure(a.n, a.runs, a.warmup)}
    print(json.dumps({k: {q: v for q, v in r.items() if not q.endswith("_ms")} for k, r in out.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
