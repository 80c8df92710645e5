#!/usr/bin/env python3
"""Device time of the Deff Hessian-vector pass (deff_sensitivity_hvp_D: k_hvp + k_pass_final, the call's own hipEvent pair)
against the field adjoint's pass (deff_field_vjp_D: k_vjp + k_pass_final) on the same context, shape and D plane, interleaved in
the same process.  The Hessian-vector pass moves 40 B per cell (four planes read, one map written) and makes three divisions
per face, the adjoint's 32 B and two: the yardstick is the adjoint's pass scaled by 40 / 32.  Reported are the SLOWEST
Hessian-vector run against that yardstick's FASTEST, beside the adjoint pass's own slowest / fastest spread in the same run.
Nothing was promised for this kernel before it was measured: the figures say where it stands.  Run on the GPU box.

  python tools/measure_hvp.py [--n 4096] [--runs 10] [--warmup 3] [--out profiles/hvp_results.json]

One context, a synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field, a random lambda, a random
dx (deff_set_tangent) and a random direction (the passes cost the same on any planes), D = the image's two diffusivities as a
plane; `warmup` calls dropped, then `runs` calls of each pass, alternating."""
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

BYTES, BYTES_VJP = 40.0, 32.0
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
        dp, ddp = D.ctypes.data_as(C.c_void_p), dD.ctypes.data_as(C.c_void_p)
        e = (C.c_double * 1)()
        ms = C.c_float()
        hvp, vjp = [], []
        for r in range(warmup + runs):
            check(s._L.deff_sensitivity_hvp_D(s._ctx, dp, ddp, 0.0, 1.0, None, e, C.byref(ms)))   # no map to the host: the device pass alone
            if r >= warmup:
                hvp.append(ms.value)
            check(s._L.deff_field_vjp_D(s._ctx, dp, 0.0, 1.0, None, e, C.byref(ms)))
            if r >= warmup:
                vjp.append(ms.value)
        plan = {k: s.plan_value(k) for k in ("hvp_kt", "hvp_items", "vjp_kt", "vjp_items")}
    slow, fast = max(hvp) * 1e-3, min(hvp) * 1e-3
    v_slow, v_fast = max(vjp) * 1e-3, min(vjp) * 1e-3
    scale = BYTES / BYTES_VJP
    ratio, spread = slow / (scale * v_fast), v_slow / v_fast
    return {"mesh": [n, n], "runs": runs, "plan": plan, "hvp_ms": hvp, "vjp_ms": vjp,
            "hvp_slowest_us": slow * 1e6, "hvp_fastest_us": fast * 1e6, "vjp_slowest_us": v_slow * 1e6, "vjp_fastest_us": v_fast * 1e6,
            "yardstick_us": scale * v_fast * 1e6,                  # the adjoint pass's fastest run x 40 / 32
            "hvp_slowest_over_yardstick": ratio, "hvp_fastest_over_yardstick": fast / (scale * v_fast),
            "vjp_slowest_over_fastest": spread, "within_vjp_spread": bool(ratio <= spread),
            "model_us_at_copy_stream": cells * BYTES / COPY_STREAM * 1e6,
            "tb_per_s_slowest": cells * BYTES / slow / 1e12, "tb_per_s_fastest": cells * BYTES / fast / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hvp_results.json"), help="'' writes no file")
    a = ap.parse_args()
    out = {f"img{a.n}": measure(a.n, a.runs, a.warmup)}
    print(json.dumps({k: {q: v for q, v in r.items() if not q.endswith("_ms")} for k, r in out.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
