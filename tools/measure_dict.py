#!/usr/bin/env python3
"""What the row dictionary harvest costs at the first sweep of an imported system -> profiles/dict_harvest.json.

Timed: the wall time of the first sweeps(1) after set_system (the field set and the stream idle before the clock starts), with
"dict" 1 and with "dict" 0, in fresh contexts, for
  2phase    the system of a random half-and-half mask (about 95 distinct rows: the harvest succeeds, the sweep runs matrix-free)
  uniform   the system of a uniform-random D plane (every row its own: at 1024^2 the hash table of 16 384 slots overflows and
            every later cell probes all of it; the sweep runs on the explicit planes)
at 1024^2, and at 2048^2 if the 1024^2 measurement took under 10 s.  Two builds of the library alternate, each in a child
process of its own (DEFF_AMD_LIB): --parent another build (the commit before a change to the harvest) and the in-tree one;
--repeats rounds of both.  The whole run is under one time limit (--limit seconds): a child gets what is left of it, and one
that fails or runs out of time ends the run.

The figure a change to k_dict_insert is judged by: parent's first call of the overflowing attempt over the same call with "dict" 0.

usage: measure_dict.py [--parent other.so] [--repeats 3] [--limit 480] [--out file]      (or, internally, --child N)
       measure_dict.py --throughput     the older figure: a 4096^2 3-phase system on the explicit kernel against its dictionary"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def systems(pkg, n):
    """name -> (A, b, D), assembled by the library itself from a D plane and exported"""
    rng = np.random.default_rng(n)
    planes = {"2phase": np.where(rng.random((n, n)) < 0.5, 1.0, 1e-2), "uniform": rng.uniform(0.5, 2.0, (n, n))}
    out = {}
    for name, D in planes.items():
        with pkg.Solver(n, n, kernel="explicit") as s:
            s.assemble_from_D(D, 0.0, 1.0)
            A, b = s.get_system()
        out[name] = (A, b, D)
    return out


def child(n):
    import effectivediffusivityfvm_amd as pkg
    # code objects loaded and both kernel families launched once before anything is timed
    for dict_on in (1, 0):
        with pkg.Solver(64, 64) as s:
            s.set_tuning("dict", dict_on)
            s.assemble_from_D(np.where(np.random.default_rng(0).random((64, 64)) < 0.5, 1.0, 1e-2), 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            s.sweeps(1)
            s.synchronize()
    res = {}
    for name, (A, b, D) in systems(pkg, n).items():
        for dict_on in (1, 0):
            with pkg.Solver(n, n) as s:
                s.set_tuning("dict", dict_on)
                t0 = time.perf_counter()
                s.set_system(A, b, D, 0.0, 1.0)
                s.synchronize()
                import_ms = (time.perf_counter() - t0) * 1e3
                s.init_linear(0.0, 1.0)
                s.synchronize()
                t0 = time.perf_counter()
                s.sweeps(1)
                s.synchronize()
                first_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                s.sweeps(1)
                s.synchronize()
                second_ms = (time.perf_counter() - t0) * 1e3
                try:
                    outcome = s.plan_value("dict_outcome")
                except pkg.DeffError:                      # a build from before the key
                    outcome = None
                res[f"{name}_dict{dict_on}"] = {"import_ms": import_ms, "first_sweeps1_ms": first_ms, "second_sweeps1_ms": second_ms,
                                                "kernel": s.kernel_in_use(), "dict_outcome": outcome}
    print("RESULT " + json.dumps(res))
    return 0


def throughput():
    import effectivediffusivityfvm_amd as pkg
    out = {}
    n = 4096
    rng = np.random.default_rng(1)
    f = np.kron(rng.random((n // 8, n // 8)), np.ones((8, 8)))
    pix = np.where(f < 0.33, 0, np.where(f < 0.66, 150, 255)).astype(np.uint8)
    grid, _ = pkg.flood_fill((pix > 200).astype(np.uint32))
    for kernel in ("explicit", "auto"):
        with pkg.Solver(n, n, kernel=kernel) as s:
            s.set_image(pix)
            t0 = time.perf_counter()
            s.assemble_3phase(0.0, 1.0, 100.0, 0.0, 1.0, grid)
            s.init_linear(0.0, 1.0)
            s.sweeps(12)
            setup = time.perf_counter() - t0
            ms = min(s.sweeps(240) for _ in range(3))
            out[f"3phase_{kernel}"] = {"kernel": s.kernel_in_use(), "us_per_sweep": ms * 1e3 / 240,
                                       "Mcells_iter_per_s": n * n * 240 / (ms * 1e-3) / 1e6, "setup_s": setup}
    print(json.dumps(out, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int)
    ap.add_argument("--throughput", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=float, default=480.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_harvest.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if a.throughput:
        return throughput()
    deadline = time.monotonic() + a.limit
    builds = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("branch", None)]
    out = {"repeats": a.repeats, "builds": [b for b, _ in builds], "sizes": {}}
    for n in (1024, 2048):
        runs = {b: [] for b, _ in builds}
        t_size = time.monotonic()
        for _ in range(a.repeats):
            for build, lib in builds:
                env = dict(os.environ)
                env.pop("DEFF_AMD_LIB", None)
                if lib:
                    env["DEFF_AMD_LIB"] = lib
                left = deadline - time.monotonic()
                if left <= 1:
                    print(f"{n}: the run's time limit of {a.limit:.0f} s is used up; stopping", flush=True)
                    return 1
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n)], env=env, capture_output=True,
                                       text=True, timeout=left)
                except subprocess.TimeoutExpired:
                    print(f"{n} {build}: not finished within the run's time limit; stopping", flush=True)
                    return 1
                if r.returncode != 0:
                    print(f"{n} {build}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return 1
                runs[build].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
                print(f"{n} {build}: done", flush=True)
        took = time.monotonic() - t_size
        size = {"measurement_s": took}
        for build, rs in runs.items():
            size[build] = {}
            for case in rs[0]:
                first = [q[case]["first_sweeps1_ms"] for q in rs]
                size[build][case] = {"first_sweeps1_ms": first, "median_ms": statistics.median(first),
                                     "second_sweeps1_ms": [q[case]["second_sweeps1_ms"] for q in rs],
                                     "import_ms": [q[case]["import_ms"] for q in rs],
                                     "kernel": rs[0][case]["kernel"], "dict_outcome": rs[0][case]["dict_outcome"]}
            for name in ("2phase", "uniform"):
                size[build][f"{name}_first_call_dict1_over_dict0"] = (size[build][f"{name}_dict1"]["median_ms"]
                                                                      / size[build][f"{name}_dict0"]["median_ms"])
        out["sizes"][str(n)] = size
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
        if took >= 10.0 * a.repeats * len(builds):
            print(f"{n}: {took:.1f} s for {a.repeats * len(builds)} runs (10 s each or more): the next size is not run", flush=True)
            break
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
