#!/usr/bin/env python3
"""Device time of the field tangent's pass (deff_tangent_rhs_D: k_tan + k_pass_final, the call's own hipEvent pair) against the
field adjoint's pass (deff_field_vjp_D: k_vjp + k_pass_final) on the same context, shape and D plane, interleaved in the same
process.  Both move 32 B per cell (three planes read, one map written) and make two divisions per face, so the adjoint's pass
is the yardstick: reported are the SLOWEST tangent run against the FASTEST adjoint run.  Run on the GPU box.

  python tools/measure_tangent.py [--n 4096] [--runs 10] [--warmup 3] [--out profiles/tangent_results.json]

One context, a synthetic 2-phase image system (seed 12345, Ds 1e-3), the linear guess as the field, a random lambda and a random
direction (the passes cost the same on any field), D = the image's two diffusivities as a plane; `warmup` calls dropped, then
`runs` calls of each pass, alternating."""
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
MARGIN = 1.10                                          # the adjoint pass's run-to-run spread (3 %) + the extra multiply-adds per face


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
        dp, ddp = D.ctypes.data_as(C.c_void_p), dD.ctypes.data_as(C.c_void_p)
        e = (C.c_double * 1)()
        ms = C.c_float()
        tan, vjp = [], []
        for r in range(warmup + runs):
            check(s._L.deff_tangent_rhs_D(s._ctx, dp, ddp, 0.0, 1.0, None, e, C.byref(ms)))   # no map to the host: the device pass alone
            if r >= warmup:
                tan.append(ms.value)
            check(s._L.deff_field_vjp_D(s._ctx, dp, 0.0, 1.0, None, e, C.byref(ms)))
            if r >= warmup:
                vjp.append(ms.value)
        plan = {k: s.plan_value(k) for k in ("tan_kt", "tan_items", "vjp_kt", "vjp_items")}
    slow, fast = max(tan) * 1e-3, min(tan) * 1e-3
    v_slow, v_fast = max(vjp) * 1e-3, min(vjp) * 1e-3
    return {"mesh": [n, n], "runs": runs, "plan": plan, "tan_ms": tan, "vjp_ms": vjp,
            "tan_slowest_us": slow * 1e6, "tan_fastest_us": fast * 1e6, "vjp_slowest_us": v_slow * 1e6, "vjp_fastest_us": v_fast * 1e6,
            "tan_slowest_over_vjp_fastest": slow / v_fast, "tan_fastest_over_vjp_fastest": fast / v_fast,
            "within_margin": bool(slow <= MARGIN * v_fast),
            "model_us_at_copy_stream": cells * BYTES / COPY_STREAM * 1e6,
            "tb_per_s_slowest": cells * BYTES / slow / 1e12, "tb_per_s_fastest": cells * BYTES / fast / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_results.json"), help="'' writes no file")
    a = ap.parse_args()
    out = {f"img{a.n}": measure(a.n, a.runs, a.warmup)}
    print(json.dumps({k: {q: v for q, v in r.items() if not q.endswith("_ms")} for k, r in out.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
