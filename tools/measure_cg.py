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
onchip_config1   00000.jpg 128^2 in a one-image context: the streaming kernels ("cg_onchip" 0: the code path every earlier
              revision runs) against the on-chip kernel ("cg_onchip" 1), alternating, 10 runs each at check_every 64 and 512
onchip_stack256  256 synthetic 128^2 images (seed 12345, images 0-255) in one stack: the same comparison, --runs times each
              at check_every 64 and 512; loop_ms, per-iteration time, ratio fastest streaming / slowest on-chip
onchip_dataset   tools/measure_dataset.py's 128^2 JPEG set (--images N) through deff2d: --solver cg one image at a time (what
              every earlier revision does) against --solver cg --cg-batch 1024, --runs times each, and the Jacobi streaming
              slots once; images/s
onchip_profile   k_cg_image's share of loop_ms from a `rocprofv3 --kernel-trace --stats` run of its own (a child process)
  python tools/measure_cg.py --cases onchip_config1,onchip_stack256,onchip_dataset,onchip_profile --out profiles/cg_onchip_results.json
stream_library   --images N (4096) synthetic 128^2 images, host pixels, upload included, whole-call wall clock: (a) consecutive
              deff_solve_cg stacks of B = deff_recommended_batch images with "cg_onchip" 1 at check_every 64 and 512 (what
              --cg-batch does) against (b) deff_solve_cg_stream through B slots at check_every 64; the forms alternate run by
              run on fresh contexts; CU-busy share = sum of iterations x --per-iter-us / (wall x min(B, compute units))
stream_profile   where the stream's time goes: a `rocprofv3 --kernel-trace --stats` run of its own (a child process) of the stream alone
stream_driver    tools/measure_dataset.py's JPEG set through deff2d: --solver cg --cg-batch 1024 against --cg-stream B, alternating
  python tools/measure_cg.py --cases stream_library,stream_driver --images 4096 --out profiles/cg_stream_results.json
slabs4096     bench4096's image and rtol: one context (deff_solve_cg) against 1, 2 and 4 row slabs on ONE GPU
              (deff_slab_group_solve_cg), the four forms alternating, --runs rounds; iterations to rtol, loop_ms, time per
              iteration.  One slab = what the slab kernels cost; 2 and 4 = the exchange and the gathers per iteration
  python tools/measure_cg.py --cases slabs4096 --runs 2 --out profiles/cg_slabs_results.json
planes_iter    the plane form ("cg_planes", kernels_cg_planes.hpp) per iteration at 1024^2 and 4096^2, a fixed number of iterations
              (rtol 0): a diffusivity drawn cell by cell (uniform 0.5 ... 2, assemble_from_D, key 1) and the native benchmark
              image under key 2 next to key 0 in the same process, alternating, --runs times; against the bytes models
              (136 B/cell on planes, 68 B/cell on the table) at 4.7 and 6.3 TB/s
planes_to_rtol the per-cell D at 1024^2 to --rtol on planes, next to what such a system could do before: deff_solve on the
              explicit kernel to tol 1e-6
planes_profile the per-kernel split of the 4096^2 per-cell-D run: a `rocprofv3 --kernel-trace --stats` run of its own (a child
              process); --stats-out keeps the table
  python tools/measure_cg.py --cases planes_iter,planes_to_rtol,planes_profile --out profiles/cg_planes_results.json \
                             --stats-out profiles/cg_planes_kernel_stats.csv
fold_iter      the tuning key "cg_fold" (kernels_cg_fold.hpp) per iteration: keys 0 / 1 / 2 alternating in one process on one
              context, a fixed number of iterations at rtol 0, --runs times each, best and spread; 00000.jpg 128^2, synthetic
              1024^2 and 4096^2, the 16 x 1024^2 stack, a per-cell D at 1024^2 on planes (keys 0 / 1), 00042.jpg's final stage
fold_profile   the per-kernel split of keys 0 / 1 / 2 at 1024^2 and at 4096^2: one `rocprofv3 --kernel-trace --stats` run of its
              own per size (child processes); --stats-out keeps the two tables in one file
  python tools/measure_cg.py --cases fold_iter,fold_profile --out profiles/cg_fold_results.json \
                             --stats-out profiles/cg_fold_kernel_stats.csv
onchip_planes  systems on coefficient planes at 128^2 (a seeded per-cell D, uniform 0.5 ... 2, reproducible without any image):
              one image, a stack of 32 and a stack of 256; solve_cg and solve_adjoint to --rtol at check_every 64 and 512; the
              streaming plane kernels ("cg_onchip_planes" 0: the code path every earlier revision runs) against one image per
              compute unit (1), alternating run by run on fresh contexts, at least 3 runs each; every run's loop_ms and
              iterations, per-iteration time, ratio fastest key 0 / slowest key 1
onchip_planes_profile  k_cgp_image's share of loop_ms on the 256-image stack from a `rocprofv3 --kernel-trace --stats` run of its
              own (a child process), and the bytes it moves per compute unit against the 72 B/cell model
  python tools/measure_cg.py --cases onchip_planes,onchip_planes_profile --out profiles/cg_onchip_planes_results.json
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


def slabs4096(rtol, max_iter, runs, n=4096):
    forms = [("one_context", 0), ("slabs1", 1), ("slabs2", 2), ("slabs4", 4)]
    rows = {name: [] for name, _ in forms}
    for _ in range(runs):
        for name, k in forms:
            s = pkg.Solver(n, n) if k == 0 else pkg.SlabGroup(n, n, [0] * k)
            with s:
                s.synth_image(12345, 0)
                s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                s.init_linear(0.0, 1.0)
                t0 = time.perf_counter()
                r = s.solve_cg(rtol=rtol, max_iter=max_iter, fluxes=False)
                row = cg_row(r, n * n)
                row["wall_s"] = time.perf_counter() - t0
                rows[name].append(row)
    out = {"mesh": [n, n], "rtol": rtol, "runs": runs, "forms": rows}
    base = min(r["per_iter_us"] for r in rows["one_context"])
    out["per_iter_us_best"] = {name: min(r["per_iter_us"] for r in rows[name]) for name, _ in forms}
    out["per_iter_over_one_context"] = {name: v / base for name, v in out["per_iter_us_best"].items()}
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


def onchip_pair(make, B, rtol, max_iter, runs, check_everys, only_onchip=False):
    """Streaming kernels ("cg_onchip" 0: the code path every earlier revision runs) against one image per compute unit
    ("cg_onchip" 1) on fresh contexts, the two forms alternating run by run, at the same check_every; per check_every the
    runs, and the ratio fastest streaming / slowest on-chip loop_ms (the bar: > 1)."""
    out = {}
    for ce in check_everys:
        rows = {"streaming": [], "onchip": []}
        for _ in range(runs):
            for label, on in (("streaming", 0), ("onchip", 1)):
                if only_onchip and not on:
                    continue
                with make() as s:
                    s.set_tuning("cg_onchip", on)
                    s.init_linear(0.0, 1.0)
                    rs = s.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce, fluxes=False)
                    rs = rs if isinstance(rs, list) else [rs]
                    assert s.plan_value("cg_impl") == 1 + on and all(r.converged for r in rs)
                    its = [int(r.iters) for r in rs]
                    rows[label].append({"loop_ms": rs[0].loop_ms, "max_iters": max(its), "mean_iters": sum(its) / B,
                                        "per_iter_us": 1e3 * rs[0].loop_ms / max(its), "deff_raw_image0": rs[0].deff_raw})
        if not only_onchip:
            slow_new = max(r["loop_ms"] for r in rows["onchip"])
            fast_old = min(r["loop_ms"] for r in rows["streaming"])
            rows["slowest_onchip_ms"], rows["fastest_streaming_ms"] = slow_new, fast_old
            rows["ratio_fastest_streaming_over_slowest_onchip"] = fast_old / slow_new
        out[f"check_every_{ce}"] = rows
    return out


def onchip_stack256(rtol, max_iter, runs, only_onchip):
    n, B = 128, 256

    def make():
        s = pkg.Solver(n, n, nimg=B)
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        return s
    return {"mesh": [n, n], "nimg": B, "rtol": rtol, **onchip_pair(make, B, rtol, max_iter, runs, (512,) if only_onchip else (64, 512), only_onchip)}


def onchip_config1(rtol, max_iter, runs):
    """One image (00000.jpg, 128^2): short loops (milliseconds), so 10 alternating runs of each form per check_every."""
    pix = np.load(os.path.join(ROOT, "tests", "golden", "img00000_pix_stb.npy"))
    ny, nx = pix.shape

    def make():
        s = pkg.Solver(nx, ny)
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        return s
    return {"mesh": [nx, ny], "nimg": 1, "rtol": rtol, **onchip_pair(make, 1, rtol, max_iter, max(runs, 10), (64, 512))}


def onchip_profile(rtol):
    """The on-chip kernel's share of loop_ms: one on-chip solve of the 256-image stack in a child process of its own under
    `rocprofv3 --kernel-trace --stats` (check_every 512), k_cg_image's total duration against that run's loop_ms."""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable,
                            os.path.abspath(__file__), "--cases", "onchip_stack256", "--runs", "1", "--only-onchip", "--rtol", repr(rtol),
                            "--out", run], capture_output=True, text=True, timeout=600)
        if p.returncode != 0 or not os.path.exists(run):
            return {"error": (p.stderr or p.stdout)[-1500:]}
        row = json.load(open(run))["onchip_stack256"]["check_every_512"]["onchip"][0]
        out = {"loop_ms": row["loop_ms"], "max_iters": row["max_iters"], "kernels": {}}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        trace = glob.glob(os.path.join(d, "prof", "**", "*kernel_trace*.csv"), recursive=True)
        if files:
            for k in csv.DictReader(open(files[0])):
                out["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6}
        elif trace:                                                  # no stats table: add the trace's durations up
            for k in csv.DictReader(open(trace[0])):
                e = out["kernels"].setdefault(k["Kernel_Name"].split("(")[0], {"calls": 0, "total_ms": 0.0})
                e["calls"] += 1
                e["total_ms"] += (int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e6
        else:
            return {**out, "error": "no kernel stats written", "files": [os.path.relpath(f, d) for f in
                                                                          glob.glob(os.path.join(d, "prof", "**", "*"), recursive=True)][:20]}
        img = [v for n_, v in out["kernels"].items() if "k_cg_image" in n_]
        if img:
            out["k_cg_image_ms"] = img[0]["total_ms"]
            out["k_cg_image_share_of_loop"] = img[0]["total_ms"] / row["loop_ms"]
            out["k_cg_image_us_per_iteration"] = 1e3 * img[0]["total_ms"] / row["max_iters"]
    return out


def onchip_dataset(rtol, runs, images):
    """tools/measure_dataset.py's images (8 x 8-pixel grains, seed 0) and input file, through the driver."""
    from PIL import Image
    exe = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
    S = 128
    out = {"image_size": S, "images": images, "cg_rtol": rtol, "runs": {}}
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(0)
        for k in range(images):
            f = np.kron(rng.random((S // 8, S // 8)), np.ones((8, 8)))
            Image.fromarray(np.where(f < rng.uniform(0.45, 0.75), 0, 255).astype(np.uint8)).save(os.path.join(d, f"{k:05d}.jpg"), quality=95)
        open(os.path.join(d, "input.txt"), "w").write(
            "Input File:\nPhases: 2\nDs: 1e-3\nDf: 1\nMeshAmpX: 1\nMeshAmpY: 1\nCR: 1\nCL: 0\nOutputName: out.csv\n"
            f"printCMap: 0\nConvergence: 1e-6\nMaxIter: 5e5\nVerbose: 0\nRunBatch: 1\nNumImages: {images}\n")
        cg = ["--solver", "cg", "--cg-rtol", repr(rtol)]
        for label, extra, n in (("cg_one_at_a_time", cg, runs), ("cg_batch_1024", cg + ["--cg-batch", "1024"], runs), ("jacobi_streaming", [], 1)):
            rows = []
            for q in range(n):
                t0 = time.perf_counter()
                p = subprocess.run([exe, "input.txt", "--json", f"{label}{q}.json"] + extra, cwd=d, capture_output=True, text=True, timeout=1200)
                dt = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr
                res = json.load(open(os.path.join(d, f"{label}{q}.json")))["results"]
                rows.append({"seconds": dt, "images_per_s": len(res) / dt, "mean_iterations": sum(x["iterations"] for x in res) / len(res),
                             "mean_Deff": sum(x["Deff"] for x in res) / len(res)})
            out["runs"][label] = rows
    slow_new = min(r["images_per_s"] for r in out["runs"]["cg_batch_1024"])
    fast_old = max(r["images_per_s"] for r in out["runs"]["cg_one_at_a_time"])
    out["slowest_batched_images_per_s"], out["fastest_one_at_a_time_images_per_s"] = slow_new, fast_old
    out["speedup_slowest_new_over_fastest_old"] = slow_new / fast_old
    return out


def synth_pixels(n, first, count, seed=12345):
    """k_synth_mask on the host: images first .. first + count - 1 of the n x n sequence, (count, n, n) uint8."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(first * n * n, (first + count) * n * n, dtype=np.uint64)) & M
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return np.where(z >> np.uint64(63), 255, 0).astype(np.uint8).reshape(count, n, n)


def stream_library(rtol, max_iter, runs, images, per_iter_us, only_stream=False):
    import torch                                                     # before the library is loaded: one HIP runtime for both
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 128
    B = pkg.recommended_batch(n, n, images)
    pix = synth_pixels(n, 0, images)
    busy = min(B, cus)                                               # compute units an on-chip launch can keep busy
    out = {"mesh": [n, n], "images": images, "slots": B, "compute_units": cus, "rtol": rtol, "per_iter_us_model": per_iter_us,
           "runs": {}}

    def row(wall, iters):
        return {"wall_s": wall, "images_per_s": images / wall, "mean_iters": sum(iters) / len(iters), "max_iters": max(iters),
                "cu_busy_share": sum(iters) * per_iter_us * 1e-6 / (wall * busy)}

    def stacks(ce):
        t0 = time.perf_counter()
        iters = []
        with pkg.Solver(n, n, nimg=B) as s:
            s.set_tuning("cg_onchip", 1)
            for k in range(0, images - images % B, B):
                s.set_image(pix[k:k + B])
                s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                s.init_linear(0.0, 1.0)
                rs = s.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce, fluxes=False)
                assert all(r.converged for r in rs) and s.plan_value("cg_impl") == 2
                iters += [int(r.iters) for r in rs]
        rest = images % B                                            # the last, shorter stack gets a context of its own, as in the driver
        if rest:
            with pkg.Solver(n, n, nimg=rest) as s:
                s.set_tuning("cg_onchip", 1)
                s.set_image(pix[images - rest:])
                s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                s.init_linear(0.0, 1.0)
                rs = s.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce, fluxes=False)
                rs = rs if isinstance(rs, list) else [rs]
                iters += [int(r.iters) for r in rs]
        return row(time.perf_counter() - t0, iters)

    def stream(ce):
        t0 = time.perf_counter()
        with pkg.Solver(n, n, nimg=B) as s:
            s.set_tuning("cg_onchip", 1)
            rs = s.solve_cg_stream(pix, 1e-3, 1.0, 0.0, 1.0, rtol=rtol, max_iter=max_iter, check_every=ce)
            assert all(r.converged for r in rs) and s.plan_value("cg_impl") == 2
            fig = {k: s.plan_value(k) for k in ("cgs_intervals", "cgs_launches", "cgs_waits")}
        return {**row(time.perf_counter() - t0, [int(r.iters) for r in rs]), **fig}

    forms = (("stacks_ce64", lambda: stacks(64)), ("stacks_ce512", lambda: stacks(512)), ("stream_ce64", lambda: stream(64)))
    for _ in range(runs):
        for label, fn in forms[2:] if only_stream else forms:
            out["runs"].setdefault(label, []).append(fn())
    if only_stream:
        return out
    slow_new = max(r["wall_s"] for r in out["runs"]["stream_ce64"])
    fast_old = min(r["wall_s"] for k in ("stacks_ce64", "stacks_ce512") for r in out["runs"][k])
    out["slowest_stream_s"], out["fastest_stacks_s"] = slow_new, fast_old
    out["ratio_fastest_stacks_over_slowest_stream"] = fast_old / slow_new
    return out


def stream_profile(rtol, images):
    """Where the stream's time goes: one stream_library run of the stream alone in a child process of its own under
    `rocprofv3 --kernel-trace --stats` (no counters in the same run); per kernel the calls and the total duration, next to
    that run's wall clock (which includes the context's creation and the tracer's own cost per launch)."""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "stream_library", "--runs", "1", "--only-stream",
                            "--images", str(images), "--rtol", repr(rtol), "--out", run], capture_output=True, text=True, timeout=600)
        if p.returncode != 0 or not os.path.exists(run):
            return {"error": (p.stderr or p.stdout)[-1500:]}
        row = json.load(open(run))["stream_library"]["runs"]["stream_ce64"][0]
        out = {"run": row, "kernels": {}}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        trace = glob.glob(os.path.join(d, "prof", "**", "*kernel_trace*.csv"), recursive=True)
        if files:
            for k in csv.DictReader(open(files[0])):
                out["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6}
        elif trace:
            for k in csv.DictReader(open(trace[0])):
                e = out["kernels"].setdefault(k["Kernel_Name"].split("(")[0], {"calls": 0, "total_ms": 0.0})
                e["calls"] += 1
                e["total_ms"] += (int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e6
        else:
            return {**out, "error": "no kernel stats written"}
        out["kernels_total_ms"] = sum(v["total_ms"] for v in out["kernels"].values())
        out["kernels_share_of_wall"] = out["kernels_total_ms"] / (1e3 * row["wall_s"])
    return out


def stream_driver(rtol, runs, images):
    """tools/measure_dataset.py's images through the driver: --cg-batch 1024 (the parent's way) against --cg-stream B."""
    from PIL import Image
    exe = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
    S = 128
    B = pkg.recommended_batch(S, S, images)
    out = {"image_size": S, "images": images, "cg_rtol": rtol, "slots": B, "runs": {}}
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(0)
        for k in range(images):
            f = np.kron(rng.random((S // 8, S // 8)), np.ones((8, 8)))
            Image.fromarray(np.where(f < rng.uniform(0.45, 0.75), 0, 255).astype(np.uint8)).save(os.path.join(d, f"{k:05d}.jpg"), quality=95)
        open(os.path.join(d, "input.txt"), "w").write(
            "Input File:\nPhases: 2\nDs: 1e-3\nDf: 1\nMeshAmpX: 1\nMeshAmpY: 1\nCR: 1\nCL: 0\nOutputName: out.csv\n"
            f"printCMap: 0\nConvergence: 1e-6\nMaxIter: 5e5\nVerbose: 0\nRunBatch: 1\nNumImages: {images}\n")
        cg = ["--solver", "cg", "--cg-rtol", repr(rtol)]
        for q in range(runs):
            for label, extra in (("cg_batch_1024", ["--cg-batch", "1024"]), ("cg_stream", ["--cg-stream", str(B)])):
                t0 = time.perf_counter()
                p = subprocess.run([exe, "input.txt", "--json", f"{label}{q}.json"] + cg + extra, cwd=d, capture_output=True, text=True, timeout=1200)
                dt = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr
                res = json.load(open(os.path.join(d, f"{label}{q}.json")))["results"]
                out["runs"].setdefault(label, []).append(
                    {"seconds": dt, "images_per_s": len(res) / dt, "mean_iterations": sum(x["iterations"] for x in res) / len(res),
                     "mean_Deff": sum(x["Deff"] for x in res) / len(res)})
    slow_new = max(r["seconds"] for r in out["runs"]["cg_stream"])
    fast_old = min(r["seconds"] for r in out["runs"]["cg_batch_1024"])
    out["slowest_stream_s"], out["fastest_batch_s"] = slow_new, fast_old
    out["ratio_fastest_batch_over_slowest_stream"] = fast_old / slow_new
    return out


PLANES_BYTES_PER_CELL = 136                                    # k_cgp_dir 80 + k_cgp_update 56 ("Planes")
STREAM_TBS = (4.7, 6.3)                                         # the chip's measured read/write stream rates


def planes_row(r, cells, bytes_per_cell):
    per_it_us = 1e3 * r.loop_ms / max(1, r.iters)
    model = {f"{t}": cells * bytes_per_cell / (t * 1e12) * 1e6 for t in STREAM_TBS}
    return {"iters": int(r.iters), "loop_ms": r.loop_ms, "per_iter_us": per_it_us, "bytes_per_cell_model": bytes_per_cell,
            "model_us_at_TBs": model, "per_iter_over_model": {t: per_it_us / v for t, v in model.items()},
            "achieved_TBs_of_model_bytes": cells * bytes_per_cell / (per_it_us * 1e-6) / 1e12}


def per_cell_D(n):
    return np.random.default_rng(n).uniform(0.5, 2.0, (n, n))


def planes_iter(runs, sizes=(1024, 4096)):
    out = {}
    for n in sizes:
        iters = 400 if n <= 1024 else 100
        rows = {"per_cell_D_planes": [], "native_table": [], "native_planes": []}
        with pkg.Solver(n, n) as s:
            s.set_tuning("cg_planes", 1)
            s.assemble_from_D(per_cell_D(n), 0.0, 1.0)
            for _ in range(runs + 1):                                # the first run allocates and warms up
                s.init_linear(0.0, 1.0)
                r = s.solve_cg(rtol=0.0, max_iter=iters, check_every=iters, fluxes=False)
                assert s.plan_value("cg_impl") == 3 and r.iters == iters
                rows["per_cell_D_planes"].append(planes_row(r, n * n, PLANES_BYTES_PER_CELL))
        with pkg.Solver(n, n) as s:
            s.synth_image(12345, 0)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            for _ in range(runs + 1):
                for key, name in ((0, "native_table"), (2, "native_planes")):
                    s.set_tuning("cg_planes", key)
                    s.init_linear(0.0, 1.0)
                    r = s.solve_cg(rtol=0.0, max_iter=iters, check_every=iters, fluxes=False)
                    assert s.plan_value("cg_impl") == (3 if key else 1) and r.iters == iters
                    rows[name].append(planes_row(r, n * n, PLANES_BYTES_PER_CELL if key else BYTES_PER_CELL))
        best = {k: min(x["per_iter_us"] for x in v[1:]) for k, v in rows.items()}
        out[f"{n}x{n}"] = {"iterations_per_run": iters, "runs": {k: v[1:] for k, v in rows.items()}, "per_iter_us_best": best,
                           "planes_over_table_native": best["native_planes"] / best["native_table"]}
    return out


def planes_to_rtol(rtol, max_iter, n=1024):
    D = per_cell_D(n)
    out = {"mesh": [n, n], "rtol": rtol}
    with pkg.Solver(n, n) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 1.0)
        for _ in range(2):
            s.init_linear(0.0, 1.0)
            t0 = time.perf_counter()
            r = s.solve_cg(rtol=rtol, max_iter=max_iter, fluxes=False)
            wall = time.perf_counter() - t0
        assert s.plan_value("cg_impl") == 3
        out["cg_planes"] = {**planes_row(r, n * n, PLANES_BYTES_PER_CELL), "rel_residual": r.rel_residual,
                            "converged": bool(r.converged), "deff_raw": r.deff_raw, "wall_s": wall}
        s.init_linear(0.0, 1.0)
        t0 = time.perf_counter()
        rj = s.solve(1e-6, 5_000_000)
        out["jacobi_explicit_tol_1e-6"] = {"kernel": s.kernel_in_use(), "sweeps": rj.iters, "deff_raw": rj.deff_raw,
                                           "loop_ms": rj.loop_ms, "wall_s": time.perf_counter() - t0,
                                           "rel_residual_of_its_field": float(s.residual(D, 0.0, 1.0))}
        out["deff_gap_jacobi_to_cg"] = abs(rj.deff_raw - r.deff_raw) / abs(r.deff_raw)
        out["jacobi_loop_ms_over_cg_loop_ms"] = rj.loop_ms / r.loop_ms
    return out


def planes_profile(stats_out):
    """The per-kernel split of the plane form at 4096^2 (per-cell D): one child process under rocprofv3 --kernel-trace --stats."""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "planes_iter", "--runs", "1", "--only-planes-4096",
                            "--out", run], capture_output=True, text=True, timeout=900)
        if p.returncode != 0 or not os.path.exists(run):
            return {"error": (p.stderr or p.stdout)[-1500:]}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        if not files:
            return {"error": "no kernel stats written"}
        out = {"kernels": {}}
        for k in csv.DictReader(open(files[0])):
            out["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6,
                                                       "average_us": float(k["AverageNs"]) / 1e3, "percent": float(k["Percentage"])}
        if stats_out:
            shutil.copy(files[0], stats_out)
    return out


def fold_workloads(only=None):
    """(name, cells, bytes per cell of the model, iterations per run, keys, context with its system assembled)"""
    def synth(n, nimg=1):
        s = pkg.Solver(n, n, nimg=nimg)
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        return s

    def config1_image():
        pix = np.load(os.path.join(ROOT, "tests", "golden", "img00000_pix_stb.npy"))
        s = pkg.Solver(pix.shape[1], pix.shape[0])
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        return s

    def per_cell(n):
        s = pkg.Solver(n, n)
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(per_cell_D(n), 0.0, 1.0)
        return s

    def shipped_final_stage():
        pix = pkg.load_jpeg_gray(os.path.join(ROOT, "tests", "golden", "00042.jpg"))
        grid, _ = pkg.flood_fill((pix > 200).astype(np.uint32))
        s = pkg.Solver(pix.shape[1], pix.shape[0])
        s.set_image(pix)
        s.assemble_3phase(0.0, 1.0, 1237500.0, 0.0, 1.0, grid)
        return s

    table = [("config1_128", 2000, (0, 1, 2), BYTES_PER_CELL, config1_image),
             ("synth_1024", 400, (0, 1, 2), BYTES_PER_CELL, lambda: synth(1024)),
             ("synth_4096", 100, (0, 1, 2), BYTES_PER_CELL, lambda: synth(4096)),
             ("stack_16x1024", 100, (0, 1, 2), BYTES_PER_CELL, lambda: synth(1024, 16)),
             ("per_cell_D_1024_planes", 400, (0, 1), PLANES_BYTES_PER_CELL, lambda: per_cell(1024)),
             ("shipped_00042_final_stage", 200, (0, 1, 2), BYTES_PER_CELL, shipped_final_stage)]
    return [w for w in table if only is None or w[0] in only]


def fold_iter(runs, only=None):
    out = {}
    for name, iters, keys, bpc, make in fold_workloads(only):
        with make() as s:
            cells = s.nx * s.ny * s.nimg
            rows = {k: [] for k in keys}
            for _ in range(runs + 1):                                # the first round allocates and warms up
                for k in keys:
                    s.set_tuning("cg_fold", k)
                    s.init_linear(0.0, 1.0)
                    rs = s.solve_cg(rtol=0.0, max_iter=iters, check_every=iters, fluxes=False)
                    r = rs[0] if isinstance(rs, list) else rs
                    assert s.plan_value("cg_fold") == (min(k, 1) if s.plan_value("cg_impl") == 3 else k) and r.iters == iters
                    rows[k].append(planes_row(r, cells, bpc))
            per = {k: [x["per_iter_us"] for x in v[1:]] for k, v in rows.items()}
            best = {k: min(v) for k, v in per.items()}
            model = rows[keys[0]][0]["model_us_at_TBs"]
            out[name] = {"mesh": [s.nx, s.ny], "nimg": s.nimg, "cg_impl": s.plan_value("cg_impl"), "cg_items": s.plan_value("cg_items"),
                         "iterations_per_run": iters, "per_iter_us": {f"fold{k}": v for k, v in per.items()},
                         "per_iter_us_best": {f"fold{k}": v for k, v in best.items()},
                         "spread_us": {f"fold{k}": max(v) - min(v) for k, v in per.items()},
                         "over_fold0": {f"fold{k}": best[k] / best[keys[0]] for k in keys},
                         "model_us_at_TBs": model,
                         "best_over_model_6.3": {f"fold{k}": best[k] / model["6.3"] for k in keys}}
    return out


def fold_profile(stats_out):
    """Keys 0 / 1 / 2 kernel by kernel at 1024^2 and 4096^2: one child process under rocprofv3 --kernel-trace --stats per size."""
    import csv
    import glob
    out = {}
    lines = []
    for name in ("synth_1024", "synth_4096"):
        with tempfile.TemporaryDirectory() as d:
            run = os.path.join(d, "run.json")
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run",
                                "--", sys.executable, os.path.abspath(__file__), "--cases", "fold_iter", "--runs", "1", "--only-fold", name,
                                "--out", run], capture_output=True, text=True, timeout=900)
            if p.returncode != 0 or not os.path.exists(run):
                out[name] = {"error": (p.stderr or p.stdout)[-1500:]}
                continue
            files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
            if not files:
                out[name] = {"error": "no kernel stats written"}
                continue
            out[name] = {"runs_per_key": 2, "iterations_per_run": json.load(open(run))["fold_iter"][name]["iterations_per_run"],
                         "kernels": {}}
            text = open(files[0]).read().splitlines()
            lines += [("\"Workload\"," + text[0])] if not lines else []
            lines += [f"\"{name}\"," + t for t in text[1:]]
            for k in csv.DictReader(text):
                out[name]["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6,
                                                                 "average_us": float(k["AverageNs"]) / 1e3, "percent": float(k["Percentage"])}
    if stats_out and lines:
        open(stats_out, "w").write("\n".join(lines) + "\n")
    return out


ONCHIP_PLANES_BYTES_PER_CELL = 72      # k_cgp_image: (A) inv 8 | (B) five planes 40 | (C) inv 8, x 8 read + 8 written


def onchip_planes_D(B, n=128):
    """The seeded per-cell diffusivity of a stack of B images (uniform 0.5 ... 2) and the adjoint's right-hand side."""
    rng = np.random.default_rng(4200 + B)
    return rng.uniform(0.5, 2.0, (B * n, n)), rng.standard_normal((B * n, n))


def onchip_planes(rtol, max_iter, runs, stacks=(1, 32, 256), only_key1=False, check_everys=(64, 512)):
    """Systems on coefficient planes (a per-cell D, assemble_from_D, "cg_planes" 1) at 128^2: the streaming plane kernels
    ("cg_onchip_planes" 0: the code path every earlier revision runs) against one image per compute unit (1), on fresh
    contexts, the two alternating run by run; solve_cg from the linear guess and solve_adjoint of a seeded w, both to rtol."""
    n = 128
    out = {"mesh": [n, n], "rtol": rtol, "bytes_per_cell_model_key1": ONCHIP_PLANES_BYTES_PER_CELL,
           "bytes_per_cell_model_key0": PLANES_BYTES_PER_CELL}
    for B in stacks:
        D, w = onchip_planes_D(B, n)
        case = {}
        for ce in check_everys:
            rows = {f"{what}_key{k}": [] for what in ("solve_cg", "solve_adjoint") for k in (0, 1)}
            for _ in range(max(runs, 3)):
                for key in (0, 1):
                    if only_key1 and not key:
                        continue
                    with pkg.Solver(n, n, nimg=B) as s:
                        s.set_tuning("cg_planes", 1)
                        s.set_tuning("cg_onchip_planes", key)
                        s.assemble_from_D(D, 0.0, 1.0)
                        s.init_linear(0.0, 1.0)
                        for what in ("solve_cg", "solve_adjoint"):
                            if what == "solve_cg":
                                rs = s.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce, fluxes=False)
                            else:
                                rs = s.solve_adjoint(w, rtol=rtol, max_iter=max_iter, check_every=ce)
                            rs = rs if isinstance(rs, list) else [rs]
                            assert s.plan_value("cg_impl") == 3 + key and all(r.converged for r in rs)
                            its = [int(r.iters) for r in rs]
                            rows[f"{what}_key{key}"].append({"loop_ms": rs[0].loop_ms, "max_iters": max(its), "mean_iters": sum(its) / B,
                                                             "per_iter_us": 1e3 * rs[0].loop_ms / max(its)})
            if not only_key1:
                for what in ("solve_cg", "solve_adjoint"):
                    fast_old = min(r["loop_ms"] for r in rows[f"{what}_key0"])
                    slow_new = max(r["loop_ms"] for r in rows[f"{what}_key1"])
                    rows[f"{what}_ratio_fastest_key0_over_slowest_key1"] = fast_old / slow_new
                    rows[f"{what}_per_iter_us_best"] = {f"key{k}": min(r["per_iter_us"] for r in rows[f"{what}_key{k}"]) for k in (0, 1)}
            case[f"check_every_{ce}"] = rows
        out[f"stack{B}"] = case
    return out


def onchip_planes_profile(rtol):
    """k_cgp_image's share of loop_ms: one key-1 run of the 256-image stack (check_every 512) in a child process of its own
    under `rocprofv3 --kernel-trace --stats`."""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as d:
        run = os.path.join(d, "run.json")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "prof"), "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--cases", "onchip_planes", "--only-onchip", "--rtol", repr(rtol),
                            "--out", run], capture_output=True, text=True, timeout=600)
        if p.returncode != 0 or not os.path.exists(run):
            return {"error": (p.stderr or p.stdout)[-1500:]}
        rows = json.load(open(run))["onchip_planes"]["stack256"]["check_every_512"]
        loop_ms = sum(r["loop_ms"] for what in ("solve_cg", "solve_adjoint") for r in rows[f"{what}_key1"])
        iters = sum(r["max_iters"] for what in ("solve_cg", "solve_adjoint") for r in rows[f"{what}_key1"])
        out = {"loop_ms_all_runs": loop_ms, "max_iters_all_runs": iters, "kernels": {}}
        files = glob.glob(os.path.join(d, "prof", "**", "*kernel_stats*.csv"), recursive=True)
        if not files:
            return {**out, "error": "no kernel stats written"}
        for k in csv.DictReader(open(files[0])):
            out["kernels"][k["Name"].split("(")[0]] = {"calls": int(k["Calls"]), "total_ms": float(k["TotalDurationNs"]) / 1e6}
        img = [v for n_, v in out["kernels"].items() if "k_cgp_image" in n_]
        if img:
            out["k_cgp_image_ms"] = img[0]["total_ms"]
            out["k_cgp_image_share_of_loop"] = img[0]["total_ms"] / loop_ms
            out["k_cgp_image_us_per_iteration"] = 1e3 * img[0]["total_ms"] / iters
            out["k_cgp_image_GBs_per_CU"] = ONCHIP_PLANES_BYTES_PER_CELL * 128 * 128 / (1e3 * img[0]["total_ms"] / iters * 1e-6) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="config1,config2,bench4096,stack16x1024,shipped00042")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=2_000_000)
    ap.add_argument("--no-jacobi", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--only-onchip", action="store_true")
    ap.add_argument("--only-stream", action="store_true")
    ap.add_argument("--only-planes-4096", action="store_true")
    ap.add_argument("--only-fold", default=None, help="fold_iter: these workloads only (comma-separated)")
    ap.add_argument("--stats-out", default=None, help="planes_profile / fold_profile: where the kernel-stats table is kept")
    ap.add_argument("--per-iter-us", type=float, default=11.1, help="k_cg_image per iteration (onchip_profile), for the CU-busy share")
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
        elif case == "onchip_stack256":
            out[case] = onchip_stack256(a.rtol, a.max_iter, a.runs, a.only_onchip)
        elif case == "onchip_config1":
            out[case] = onchip_config1(a.rtol, a.max_iter, a.runs)
        elif case == "onchip_profile":
            out[case] = onchip_profile(a.rtol)
        elif case == "onchip_dataset":
            out[case] = onchip_dataset(a.rtol, a.runs, a.images)
        elif case == "stream_library":
            out[case] = stream_library(a.rtol, a.max_iter, a.runs, a.images, a.per_iter_us, a.only_stream)
        elif case == "slabs4096":
            out[case] = slabs4096(a.rtol, a.max_iter, a.runs)
        elif case == "planes_iter":
            out[case] = planes_iter(a.runs, (4096,) if a.only_planes_4096 else (1024, 4096))
        elif case == "planes_to_rtol":
            out[case] = planes_to_rtol(a.rtol, a.max_iter)
        elif case == "planes_profile":
            out[case] = planes_profile(a.stats_out)
        elif case == "fold_iter":
            out[case] = fold_iter(a.runs, a.only_fold.split(",") if a.only_fold else None)
        elif case == "fold_profile":
            out[case] = fold_profile(a.stats_out)
        elif case == "onchip_planes":
            out[case] = (onchip_planes(a.rtol, a.max_iter, 1, (256,), True, (512,)) if a.only_onchip
                         else onchip_planes(a.rtol, a.max_iter, a.runs))
        elif case == "onchip_planes_profile":
            out[case] = onchip_planes_profile(a.rtol)
        elif case == "stream_profile":
            out[case] = stream_profile(a.rtol, a.images)
        elif case == "stream_driver":
            out[case] = stream_driver(a.rtol, a.runs, a.images)
        else:
            raise SystemExit(f"unknown case {case}")
        out[case]["case_wall_s"] = time.perf_counter() - t0
        print(json.dumps({case: out[case]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
