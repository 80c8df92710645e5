#!/usr/bin/env python3
"""Headline benchmark: Mcells*iter/s of the Jacobi sweep at 4096^2 on MI355X.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]   (N > 1: starts its own N ranks as child processes)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = `--sweeps-per-step` weighted-Jacobi sweeps plus one Deff evaluation
(wall fluxes) of one synthetic two-phase image (SURVEY.md 8d generator) that is
already resident in HBM.  With N > 1 every rank solves its own image (image
index = rank): the path shards as whole images, there is no data-path
collective, scaling is weak.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times K steps, writes the last step's outputs if
--dump-outputs is given, and prints the line (headline figure and the roofline of
the timed launches).  Everything below that takes work of its own -- the
explicit-kernel, omega = 1 and contracted-arithmetic rows, the 1024^2 / 2048^2
single images, config #2 to tolerance, the residual, the live rocprofv3 child
runs and the CPU baseline with its parity check -- runs only with --full.

roofline (always a fraction of a real roof, <= 1 by construction):
  * the default kernel (temporally blocked, matrix-free) never moves the explicit operator's 64 B per
    cell per sweep and is bound by FP64 issue, so its block says bound = "fp64_valu": algorithmic flops
    = 11 FP64 add/mul per cell per sweep (7 fused in contracted arithmetic) x cells x sweeps per launch
    / the kernel's average launch duration (HIP events on the solver's own stream inside
    deff_sweeps()), against 39.3 TFLOP/s = one FP64 VALU instruction per lane per 4 clocks x 1024
    SIMDs x 2.4 GHz (the 78.6 TFLOP/s FP64 vector peak counts an FMA as two; the reference's
    written operation order has none).  Its own HBM model (x 8 + code 2 read, xNew 8 written = 18 B per
    cell per LAUNCH) is reported beside it (`hbm_own_model`).
  * the contract figure of SURVEY.md 8d -- 64 B per cell per sweep (A 5x8 + b 8 + x 8 read, xNew 8
    written: the operator behind the reference's seam) -- is measured on the explicit-coefficient
    kernel in the same run and sits in the same block: roofline.contract_64B_frac (+ _kernel,
    _launch_us, _achieved_GBs).  With --kernel explicit it IS the top-level bound ("hbm").
cpu_baseline: the single-thread CPU oracle on a bounded sample of the same workload (rank 0, N = 1
only); a reported baseline, not the target.  The field it produces is kept and the GPU field after
the same number of sweeps from the same start must be array_equal to it: "parity_checked".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
BYTES_PER_CELL_SWEEP = 64.0      # the explicit operator behind the reference seam
OWN_BYTES_PER_CELL_LAUNCH = 18.0  # matrix-free kernels: x 8 + code 2 read, xNew 8 written, per LAUNCH
# FP64 VALU: a wave64 v_add/v_mul/v_fma_f64 occupies its SIMD for 4 clocks (16 lanes/clk; tools/ubench measures 4.4)
# -> 1024 SIMDs x 16 x 2.4 GHz = 39.3 T instructions-lanes/s; an FMA counts 2 flops (78.6 TFLOP/s vector peak)
FP64_INSTR_PEAK_T = 39.3216
FP64_INSTR_PER_CELL = {False: 11, True: 7}   # tb_cell(): default arithmetic / contracted (kernels_tb.hpp)
DUMP_MAX_VALUES = 1 << 20        # --dump-outputs: an array larger than this is written as a fixed sample of this many values
DUMP_SEED = 12345


def dump_outputs(out_dir, **arrays):
    """--dump-outputs: every array as <out_dir>/<name>.npy in float64.  An array of more than DUMP_MAX_VALUES values (the
    4096^2 field) is written as the values at DUMP_MAX_VALUES positions drawn once from a generator seeded with DUMP_SEED, in
    increasing order: the same positions in every run of the same shape, at most 8 MB per array."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if a.size > DUMP_MAX_VALUES:
            pick = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, DUMP_MAX_VALUES, replace=False))
            a = a.reshape(-1)[pick]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def child_env():
    """Environment of the rocprofv3 child runs: this process's, minus what a torch.distributed launcher put there (a child
    must not join the parent's process group or bind its rendezvous port)."""
    drop = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE",
            "ROLE_NAME", "MASTER_ADDR", "MASTER_PORT", "OMP_NUM_THREADS")
    env = {k: v for k, v in os.environ.items() if k not in drop and not k.startswith("TORCHELASTIC_") and not k.startswith("TORCH_NCCL_")}
    env["TMPDIR"] = "/tmp"
    return env


def live_traffic(n, kernel, kernel_used):
    """HBM bytes per launch of the dominant sweep kernel, measured NOW: two child runs of this script under
    `rocprofv3 --pmc` (FETCH_SIZE, WRITE_SIZE; separate passes, the program itself after `--`), corrected as
    MI355X_MICROARCH.md prescribes for gfx950 (both counters in KiB; FETCH_SIZE tallies 128-B requests at 64 B: x2).
    Returns (bytes_per_launch, source) or None (no rocprofv3 / a failed child: the caller falls back to profiles/)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    want = {"matfree_tb": "k_sweep_matfree_tb", "matfree": "k_sweep_matfree<", "explicit": "k_sweep_explicit",
            "scalar": "k_sweep_scalar"}.get(kernel_used)
    if want is None:
        return None
    got = {}
    env = child_env()
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            cmd = [exe, "--pmc", ctr, "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--size", str(n), "--kernel", kernel, "--steps", "1", "--warmup", "0", "--sweeps-per-step", "24",
                   "--primary-only"]
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=240)
                files = glob.glob(os.path.join(tmp, "*", "*_counter_collection.csv"))
                if r.returncode != 0 or not files:
                    return None
                vals = [float(row["Counter_Value"]) for row in csv.DictReader(open(max(files, key=os.path.getmtime)))
                        if want in row["Kernel_Name"]]
                if not vals:
                    return None
                got[ctr] = sum(vals) / len(vals) * 1024.0
            except Exception:
                return None
    return got["FETCH_SIZE"] * 2.0 + got["WRITE_SIZE"], "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, two child runs of this command (x2 read correction, gfx950)"


def live_kernel_stats(n, kernel, kernel_used, steps, warmup, sweeps_per_step, omega, keep_as="bench_live_kernel_stats.csv"):
    """Average duration of the dominant sweep kernel as rocprofv3 sees it, measured NOW on this box: one child run of this
    script's timed region (`--primary-only`, same --steps / --warmup / --sweeps-per-step) under `rocprofv3 --kernel-trace
    --stats` (the program itself after `--`).  The summary it parses is also left in gpurun_out/ (copied to profiles/ per
    round), so that roofline.frac can be recomputed from a profile of the same box.  Returns a dict or None."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    want = {"matfree_tb": "k_sweep_matfree_tb", "matfree": "k_sweep_matfree<", "explicit": "k_sweep_explicit",
            "scalar": "k_sweep_scalar"}.get(kernel_used)
    if not os.path.exists(exe) or want is None:
        return None
    env = child_env()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--size", str(n), "--kernel", kernel, "--steps", str(steps), "--warmup", str(warmup),
               "--sweeps-per-step", str(sweeps_per_step), "--omega", repr(omega), "--primary-only"]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
            files = glob.glob(os.path.join(tmp, "*", "*_kernel_stats.csv"))
            if r.returncode != 0 or not files:
                return None
            f = max(files, key=os.path.getmtime)
            rows = [row for row in csv.DictReader(open(f)) if want in row["Name"]]
            if not rows:
                return None
            top = max(rows, key=lambda row: float(row["TotalDurationNs"]))
            keep = os.path.join(ROOT, "gpurun_out")
            if os.path.isdir(keep) and os.access(keep, os.W_OK):
                shutil.copyfile(f, os.path.join(keep, keep_as))
            child = None
            for line in r.stdout.splitlines():
                if line.startswith("{") and '"metric"' in line:
                    child = json.loads(line)
            return {"rocprof_avg_us": float(top["AverageNs"]) / 1e3, "rocprof_min_us": float(top["MinNs"]) / 1e3,
                    "rocprof_calls": int(top["Calls"]), "rocprof_share_of_gpu_time_pct": float(top["Percentage"]),
                    "rocprof_kernel": top["Name"].split("(")[0],
                    "rocprof_child_launch_us": child["roofline"]["launch_us"] if child else None,
                    "rocprof_source": "rocprofv3 --kernel-trace --stats, one child run of this command's timed region "
                                      f"(--primary-only) on this box; summary kept as gpurun_out/{keep_as}"}
        except Exception:
            return None


def iters_to_tol_1024(pkg, device, kernel):
    """The second half of BASELINE.json's metric, on config #2: ONE 1024^2 synthetic image (seed 12345, image 0, Ds 1e-3)
    by the reference's rule (relative Deff change per 10 000 sweeps < 1e-6, JacobiGPU cuh:1232-1290) through deff_solve."""
    with pkg.Solver(1024, 1024, device=device, kernel=kernel) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        t0 = time.perf_counter()
        r = s.solve(1e-6, 30_000_000)
        dt = time.perf_counter() - t0
        return {"iters": int(r.iters), "checks": int(r.checks), "deff": r.deff_raw, "conv": r.conv, "seconds": dt,
                "loop_ms": r.loop_ms, "Mcells_iter_per_s": 1024.0 * 1024.0 * r.iters / dt / 1e6, "tol": 1e-6,
                "plan": s.plan(),
                "sample": "ONE 1024x1024 synthetic image (BASELINE config #2) from the linear guess to the reference's "
                          "stopping rule, tol 1e-6, check every 10 000 sweeps, wall time of deff_solve() incl. all checks"}


def cpu_baseline(n, seconds_target=12.0, fixed_sweeps=None, with_reference_kernel=False):
    """Single-thread oracle sweep rate on the same synthetic workload (bounded sample).
    Returns (block, sweeps, field): the field after `sweeps` sweeps from the linear guess is kept so that
    the GPU path can be checked against it (parity_checked).  fixed_sweeps: SURVEY.md 8d's counts for the small configs."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_binding as ob
    ob.build()
    pix = ob.synth_mask(n, n, 12345, 0)
    D = ob.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = ob.discretize(D, 0.0, 1.0)
    x = ob.linear_guess(n, n, 0.0, 1.0)
    t0 = time.perf_counter()
    x = ob.sweeps(A, b, x, 2)
    per = (time.perf_counter() - t0) / 2
    k = fixed_sweeps or max(2, min(2000, int(seconds_target / max(per, 1e-9))))
    t0 = time.perf_counter()
    x = ob.sweeps(A, b, x, k)
    dt = time.perf_counter() - t0
    block = {"value": n * n * k / dt / 1e6, "unit": "Mcells*iter/s", "cores": 1, "kind": "port",
             "sample": f"{k} sweeps of the {n}x{n} synthetic image, oracle/deff_oracle.c (gcc -O2, AoS, 1 thread), "
                       f"host has {os.cpu_count()} logical CPUs"}
    if with_reference_kernel and ob.have_ref_kernel():
        # beside the CPU figure: the REFERENCE's own kernel (Deff2D.cuh:69-118, compiled by hipcc from its own text:
        # oracle/_ref/ref_kernel) on this GPU, launched as the reference's loop launches it -- one launch, one device
        # synchronisation and one device-to-device copy per sweep (cuh:1237-1281).  Reported, never compared as `value`;
        # its field after the same sweeps must be the oracle's bit for bit.
        try:
            x0 = ob.linear_guess(n, n, 0.0, 1.0)
            xr, ms = ob.ref_sweeps(A, b, x0, 40, timing=True, tmpdir="/tmp")
            same = bool(__import__("numpy").array_equal(xr, ob.sweeps(A, b, x0, 40)))
            block["reference_kernel_on_this_gpu"] = {
                "value": n * n * 40 / (ms * 1e-3) / 1e6, "unit": "Mcells*iter/s", "us_per_sweep": ms * 1e3 / 40, "kind": "reference",
                "bit_identical_to_oracle": same,
                "sample": "40 sweeps: updateX_SOR as written by the reference, hipcc --offload-arch=gfx950 -O2 -ffp-contract=off, grid "
                          "n/160+1 x 160, launch + hipDeviceSynchronize + D2D copy per sweep like cuh:1237-1281 (HIP events around the loop)"}
        except Exception as e:                                        # noqa: BLE001 -- a baseline leg must not fail the bench
            block["reference_kernel_on_this_gpu"] = {"error": str(e)[:200]}
    return (block, k + 2, x)


def bench_slab_one_gpu(args, pkg, torch, local_rank):
    """--mode slab --slabs N on ONE GPU: the same image as N row slabs driven by one process (peer copies between the
    slabs' buffers), with the exchange overlapped with the interior of the pass (and, with --full, without, next to the
    unsplit context).
    The slabs share the GPU, so this measures what the slab machinery and the exposed part of the exchange COST per pass,
    not a speed-up."""
    n, S, N = args.size, args.sweeps_per_step, args.slabs
    out = {}

    def run(obj):
        for _ in range(args.warmup):
            obj.sweeps(S, args.omega)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            obj.sweeps(S, args.omega)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    # the headline: the slabs with the exchange overlapped; the unsplit context and the serial exchange only with --full
    for tag, ov in (("slabs_overlap", 2),) + ((("slabs_serial", 0),) if args.full else ()):
        with pkg.SlabGroup(n, n, [local_rank] * N) as g:
            g.set_tuning("slab_overlap", ov)
            g.synth_image(12345, 0)
            g.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            g.init_linear(0.0, 1.0)
            out[tag] = run(g)
            if tag == "slabs_overlap" and args.dump_outputs:
                dump_outputs(args.dump_outputs, field=g.get_field())
    cells = float(n) * n
    line = {
        "metric": f"Mcells*iter/s (Jacobi sweep) at {n}^2, {N} row slabs on one GPU", "value": cells * S / out["slabs_overlap"] / 1e6,
        "unit": "Mcells*iter/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": out["slabs_overlap"] * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"ONE {n}x{n} synthetic two-phase image as {N} row slabs on one GPU (one process, peer copies), "
                               f"8-row halos, one exchange per temporally blocked pass; step = {S} sweeps", "sweeps_per_step": S}}
    if args.full:
        with pkg.Solver(n, n, device=local_rank) as s:
            s.synth_image(12345, 0)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            out["one_context"] = run(s)
            launches, T = s.last_launches()
        passes = S // T + S % T
        line["config"]["workload"] = line["config"]["workload"].replace("temporally blocked pass", f"pass of {T} sweeps")
        line["per_pass_us"] = {k: v / passes * 1e6 for k, v in out.items()}
        line["exchange_exposed_us_per_pass"] = {"overlapped": (out["slabs_overlap"] - out["one_context"]) / passes * 1e6,
                                                "serial": (out["slabs_serial"] - out["one_context"]) / passes * 1e6}
        line["Mcells_iter_per_s"] = {k: cells * S / v / 1e6 for k, v in out.items()}
    print(json.dumps(line), flush=True)


def bench_slab(args, pkg, torch, dist, world, rank, local_rank, barrier, use_dist, gather_elapsed):
    """One --size x --size image split into `world` row slabs (RCCL halo exchange per blocked pass)."""
    if world == 1 and args.slabs > 1:
        return bench_slab_one_gpu(args, pkg, torch, local_rank)
    n, S = args.size, args.sweeps_per_step
    if args.transport == "host" and use_dist:
        s = pkg.SlabRank(n, n, rank, world, None, device=local_rank, transport=pkg.TorchDistTransport())
    else:
        uid = [pkg.rccl_unique_id() if rank == 0 else None]
        if use_dist:
            dist.broadcast_object_list(uid, src=0)
        s = pkg.SlabRank(n, n, rank, world, uid[0], device=local_rank)
    for kv in args.tune:
        k, v = kv.split("=")
        s.set_tuning(k, int(v))
    s.synth_image(12345, 0)
    s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
    s.init_linear(0.0, 1.0)
    for _ in range(args.warmup):
        s.sweeps(S, args.omega)
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s.sweeps(S, args.omega)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank_ms = [elapsed / args.steps * 1e3]
    if use_dist:
        every = gather_elapsed(elapsed)
        per_rank_ms = [t / args.steps * 1e3 for t in every]
        elapsed = max(every)
    if args.dump_outputs:
        field = s.get_field()                       # this rank's own rows of the image after the last step
        if rank == 0:
            dump_outputs(args.dump_outputs, field=field)
    if rank == 0:
        cells = float(n) * n
        print(json.dumps({
            "per_rank_ms_per_step": per_rank_ms,
            "metric": f"Mcells*iter/s (Jacobi sweep) at {n}^2, row slabs", "value": cells * S * args.steps / elapsed / 1e6,
            "unit": "Mcells*iter/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"ONE {n}x{n} synthetic two-phase image split into {world} row slabs, 8-row halos, "
                                   f"{'host-staged (gloo)' if args.transport == 'host' else 'RCCL'} send/recv once per temporally blocked pass; step = {S} sweeps"
                                   + ("; REHEARSAL: the ranks share GPUs" if args.share_gpu else ""),
                       "kernel": "matfree_tb", "sweeps_per_step": S, "transport": args.transport}}), flush=True)
    s.close()
    if use_dist:
        barrier()
        dist.destroy_process_group()


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py <same arguments>` as a CHILD process (the form the driver itself
    uses), pass its output through and return its exit code.  The parent has not imported torch and never touches the
    GPU, and nothing is exec'ed: every rank is a fresh process."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.run(cmd, env=env).returncode


def launch_dry(world, rank, local_rank):
    """--launch-dry: prove the launcher without GPUs.  Every rank joins a gloo group on the rendezvous the launcher set
    up, the ranks gather (rank, world, local_rank, pid, parent pid) and rank 0 prints them as one JSON line."""
    import datetime
    import torch.distributed as dist
    if world > 1 or "MASTER_ADDR" in os.environ:
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
        every = [None] * world
        dist.all_gather_object(every, {"rank": rank, "world": world, "local_rank": local_rank, "pid": os.getpid(),
                                       "ppid": os.getppid()})
        dist.barrier()
        dist.destroy_process_group()
    else:
        every = [{"rank": rank, "world": world, "local_rank": local_rank, "pid": os.getpid(), "ppid": os.getppid()}]
    if rank == 0:
        print(json.dumps({"launch_dry": True, "n_gpus": world, "ranks": every}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--sweeps-per-step", type=int, default=1200)   # multiple of every T
    ap.add_argument("--kernel", default="auto", choices=["auto", "explicit", "scalar", "matfree", "matfree_tb"])
    ap.add_argument("--omega", type=float, default=2.0 / 3.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--primary-only", action="store_true", help="only the timed steps of the primary kernel: no explicit / "
                                                                "omega-1 / contracted / small-image / CPU legs (counter runs)")
    ap.add_argument("--no-live-traffic", action="store_true", help="take roofline.traffic from profiles/traffic.json instead of "
                                                                   "measuring it now (two rocprofv3 --pmc child runs)")
    ap.add_argument("--no-small-image", action="store_true", help="skip the ONE-1024^2-image row (profiling runs: its "
                                                                  "launches would mix into the per-kernel averages)")
    ap.add_argument("--no-live-stats", action="store_true", help="skip the rocprofv3 --kernel-trace --stats child run")
    ap.add_argument("--no-iters-to-tol", action="store_true", help="skip config #2's solve to tolerance (~2.5 s)")
    ap.add_argument("--explicit-sweeps", type=int, default=300,
                    help="sweeps of the secondary explicit-coefficient measurement (0 = skip)")
    ap.add_argument("--tune", action="append", default=[], help="key=value tuning knob (repeatable)")
    ap.add_argument("--mode", default="images", choices=["images", "slab"],
                    help="images: one image per GPU, no collective (default, weak scaling); slab: ONE image of "
                         "--size rows split into row slabs over the GPUs with RCCL halo exchange (config #4, strong)")
    ap.add_argument("--batch", type=int, default=1, help="images per GPU swept together (dataset-generation mode)")
    ap.add_argument("--slabs", type=int, default=1, help="--mode slab on ONE GPU: split the image into this many slabs "
                                                         "(one process, peer copies) and report the exchange's exposed time")
    ap.add_argument("--transport", default="rccl", choices=["rccl", "host"],
                    help="N > 1: rccl = torch.distributed 'nccl' backend (RCCL over xGMI; the slabs' halo exchange is grouped "
                         "ncclSend/ncclRecv) -- the product path; host = gloo + host-staged halo blocks (TorchDistTransport): "
                         "for rehearsals on boxes where RCCL cannot connect the ranks")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal on a box with fewer GPUs than ranks: rank r uses device r mod (GPUs present); needs "
                         "--transport host (RCCL refuses two ranks on one device); the ranks then SHARE a GPU, so the line's "
                         "value says nothing about scaling")
    ap.add_argument("--launch-dry", action="store_true", help="start the ranks, join a gloo group, report rank/world and "
                                                              "exit: the launcher's test (no GPU needed)")
    ap.add_argument("--full", action="store_true", help="also run every secondary measurement and check (explicit / omega-1 / "
                                                        "contracted rows, small images, tolerance solve, residual, rocprofv3 "
                                                        "children, CPU baseline and parity); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float64; the field as a "
                         "fixed seeded sample when it has more than 2^20 values)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.primary_only or not args.full:
        args.no_cpu_baseline = args.no_small_image = args.no_live_traffic = args.no_live_stats = args.no_iters_to_tol = True
        args.explicit_sweeps = 0

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: this process becomes a launcher and nothing else (it never imports torch or
        # touches HIP); the N ranks are fresh children of a torch.distributed.run child
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    if args.launch_dry:
        return launch_dry(world, rank, local_rank)

    import torch  # first: one HIP runtime for torch and libdeff_amd
    import torch.distributed as dist

    ndev = torch.cuda.device_count()          # counting devices does not initialise the GPU
    if args.share_gpu and world > 1 and args.transport != "host":
        sys.exit("bench.py: --share-gpu needs --transport host (RCCL refuses two ranks on one device)")
    if args.share_gpu and ndev > 0:
        local_rank = local_rank % ndev        # rehearsal: the ranks share the GPUs that are there
    if local_rank >= ndev:
        sys.exit(f"bench.py rank {rank}: device {local_rank} of {ndev} (this box has fewer GPUs than --gpus {world}; "
                 "there is no CPU fallback)")
    import effectivediffusivityfvm_amd as pkg

    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    # under torch.distributed.run (any N, also N = 1) use the process group: RCCL over xGMI
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_ADDR" in os.environ)
    host_transport = args.transport == "host"
    if use_dist:
        if host_transport:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    def barrier():
        if use_dist:
            if host_transport:
                dist.barrier()
            else:
                dist.barrier(device_ids=[local_rank])

    def gather_elapsed(elapsed):
        """every rank's own time (a slow rank must be visible in the line); max = all_reduce(MAX)"""
        mine = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if host_transport else "cuda")
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        return [float(t.item()) for t in every]

    # N > 1: the scaling line needs the timed steps only; the secondary legs (explicit kernel, omega = 1, contracted arithmetic,
    # small images, residual, CPU baseline) are rank 0's business at N = 1 and would only keep the other ranks waiting
    lean = args.primary_only or not args.full or world > 1
    if world > 1:
        args.explicit_sweeps = 0
        args.no_small_image = args.no_iters_to_tol = args.no_cpu_baseline = True
    n, S = args.size, args.sweeps_per_step
    if args.mode == "slab":
        return bench_slab(args, pkg, torch, dist, world, rank, local_rank, barrier, use_dist, gather_elapsed)
    s = pkg.Solver(n, n, device=local_rank, kernel=args.kernel, nimg=args.batch)
    for kv in args.tune:
        k, v = kv.split("=")
        s.set_tuning(k, int(v))
    s.synth_image(12345, rank * args.batch)     # image index = rank (x batch): independent images, no comm
    s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
    s.init_linear(0.0, 1.0)

    last = {}                                   # what the last step returned to its caller (--dump-outputs)

    def step():
        ms = s.sweeps(S, args.omega)
        deff, MFL, MFR = s.flux()
        last.update(deff=deff, MFL=MFL, MFR=MFR)
        return ms, (deff if args.batch == 1 else float(deff[0]))

    for _ in range(args.warmup):
        step()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kernel_ms = 0.0
    deff = float("nan")
    for _ in range(args.steps):
        ms, deff = step()
        kernel_ms += ms
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank_ms = [elapsed / args.steps * 1e3]
    if use_dist:
        every = gather_elapsed(elapsed)
        per_rank_ms = [t / args.steps * 1e3 for t in every]
        elapsed = max(every)
    if args.dump_outputs and rank == 0:
        # before any secondary leg sweeps the field further: Deff and wall fluxes of the last step, the field it left
        dump_outputs(args.dump_outputs, deff=last["deff"], mfl=last["MFL"], mfr=last["MFR"], field=s.get_field())

    launches, sweeps_per_launch = s.last_launches()     # of the last step
    kernel_used = s.kernel_in_use()
    plan = s.plan() if kernel_used == "matfree_tb" else None

    # Secondary, untimed-by-the-driver leg: the explicit-coefficient kernel, i.e. the
    # operator exactly as it sits behind the reference's seam (A, b streamed: 64 B/cell/sweep).
    explicit = None
    if args.explicit_sweeps > 0 and kernel_used != "explicit":
        s.set_kernel("explicit")
        s.sweeps(20, args.omega)
        ems = s.sweeps(args.explicit_sweeps, args.omega)
        explicit = (ems * 1e-3 / args.explicit_sweeps, s.kernel_in_use())
        s.set_kernel(args.kernel)

    # second reported row: plain Jacobi, omega = 1 (updateX_V1's arithmetic), same kernel
    omega1_ms = None
    if abs(args.omega - 1.0) > 1e-12 and not lean:
        s.sweeps(sweeps_per_launch * 4, 1.0)
        omega1_ms = s.sweeps(S, 1.0)

    # third reported row: the same sweeps in contracted arithmetic (opt-in "fma" mode: products fused
    # into adds as a compiler contracts the reference's expression; bit-identical to the oracle's fma
    # build, NOT to the default arithmetic -- reported beside `value`, never as `value`)
    fma_ms = None
    if kernel_used != "explicit" and not lean:
        s.set_tuning("fma", 1)
        s.sweeps(sweeps_per_launch * 4, args.omega)
        fma_ms = s.sweeps(S, args.omega)
        s.set_tuning("fma", 0)

    # fourth reported row: BASELINE config #2's shape -- ONE 1024^2 image (too few cells to fill the chip with one wave
    # per tile: the planner switches to workgroup tiles, kernels_wgtile.hpp); same physics, its own small context
    small = None
    if rank == 0 and n != 1024 and args.batch == 1 and not args.no_small_image:
        with pkg.Solver(1024, 1024, device=local_rank, kernel=args.kernel) as s2:
            s2.synth_image(12345, 0)
            s2.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s2.init_linear(0.0, 1.0)
            s2.sweeps(960, args.omega)
            ms2 = min(s2.sweeps(4800, args.omega) for _ in range(3))
            small = (1024.0 * 1024.0 * 4800 / (ms2 * 1e-3) / 1e6, s2.kernel_in_use(), s2.plan())
    # fifth row: ONE 2048^2 image -- the middle of the size range, where the planner keeps the image resident on tall
    # workgroup tiles (kernels_wgtile.hpp) instead of streaming it
    mid = None
    if rank == 0 and n != 2048 and args.batch == 1 and not args.no_small_image:
        with pkg.Solver(2048, 2048, device=local_rank, kernel=args.kernel) as s3:
            s3.synth_image(12345, 0)
            s3.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s3.init_linear(0.0, 1.0)
            s3.sweeps(480, args.omega)
            ms3 = min(s3.sweeps(2400, args.omega) for _ in range(3))
            mid = (2048.0 * 2048.0 * 2400 / (ms3 * 1e-3) / 1e6, s3.kernel_in_use(), s3.plan())

    tol1024 = None
    if rank == 0 and world == 1 and args.batch == 1 and not args.no_iters_to_tol:
        tol1024 = iters_to_tol_1024(pkg, local_rank, args.kernel)

    # Residual() of the reference (cuh:451-494) as a wave-level reduction over the field (kernels_residual.hpp): device time of
    # one evaluation and its HBM fraction against the algorithmic 9 B per cell (x 8 + pixel 1; no D plane is read)
    resid = None
    if rank == 0 and args.batch == 1 and not lean:
        t = sorted(s.residual(timing=True)[1] for _ in range(12))
        rbytes = 9.0 * float(n) * n
        resid = {"value": s.residual(), "device_us": t[0] * 1e3, "median_us": t[len(t) // 2] * 1e3,
                 "algorithmic_bytes": rbytes, "achieved_GBs": rbytes / (t[0] * 1e-3) / 1e9,
                 "frac_of_hbm_peak": rbytes / (t[0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                 "sample": "deff_residual() on the field the timed steps left: k_residual_classes + k_residual_final, HIP events, "
                           "best / median of 12; 9 B per cell (x 8 + pixel 1)"}

    if rank == 0:
        cells = float(n) * n * args.batch
        total_launches = args.steps * launches
        launch_s = kernel_ms * 1e-3 / total_launches      # avg duration of one sweep-kernel launch (HIP events)

        def traffic_of(kname):
            tfile = os.path.join(ROOT, "profiles", "traffic.json")
            try:
                return json.load(open(tfile)).get(f"{kname}_{n}")
            except Exception:
                return None

        if kernel_used in ("matfree", "matfree_tb"):
            own = OWN_BYTES_PER_CELL_LAUNCH * cells
            own_block = {"bound": "hbm", "bytes_per_launch": own, "achieved": own / launch_s / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": own / launch_s / 1e9 / HBM_PEAK_GBS,
                         "model": "x 8 + row code 2 read, xNew 8 written = 18 B per cell per LAUNCH (the coefficients "
                                  "come from a 16-bit code through the row dictionary in LDS, never from HBM)"}
        if kernel_used == "matfree_tb":
            ipc = FP64_INSTR_PER_CELL[False]
            flops = ipc * cells * sweeps_per_launch
            ach = flops / launch_s / 1e12
            roofline = {
                "bound": "fp64_valu", "achieved": ach, "peak": FP64_INSTR_PEAK_T, "unit": "TFLOP/s",
                "frac": ach / FP64_INSTR_PEAK_T, "traffic": None, "kernel": kernel_used,
                "launch_us": launch_s * 1e6, "sweeps_per_launch": sweeps_per_launch,
                "algorithmic_flops_per_launch": flops,
                "model": f"{ipc} FP64 add/mul per cell per sweep (reference operation order, no FMA: kernels_tb.hpp tb_cell) x "
                         f"cells x {sweeps_per_launch} sweeps per launch; peak = one FP64 VALU instruction per lane per 4 "
                         "clocks x 1024 SIMDs x 2.4 GHz = 39.3 T/s (half the 78.6 TFLOP/s FMA-counted vector peak); "
                         "recomputed halo cells are NOT counted",
                "hbm_own_model": own_block,
            }
        elif kernel_used == "matfree":
            roofline = dict(own_block, traffic=None, kernel=kernel_used, launch_us=launch_s * 1e6)
        else:
            alg_bytes = BYTES_PER_CELL_SWEEP * cells * sweeps_per_launch
            ach = alg_bytes / launch_s / 1e9
            roofline = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": ach / HBM_PEAK_GBS, "traffic": None, "kernel": kernel_used,
                        "launch_us": launch_s * 1e6, "algorithmic_bytes_per_launch": alg_bytes,
                        "model": "64 B per cell per sweep (A 40 + b 8 + x 8 read, xNew 8 written: the explicit "
                                 "operator behind the reference seam, SURVEY.md 8d)",
                        "contract_64B_frac": ach / HBM_PEAK_GBS, "contract_64B_kernel": kernel_used,
                        "contract_64B_launch_us": launch_s * 1e6, "contract_64B_achieved_GBs": ach}
        live = None
        if world == 1 and args.batch == 1 and not args.no_live_traffic:
            live = live_traffic(n, args.kernel, kernel_used)
        tr = traffic_of(kernel_used)
        if live:
            roofline["traffic"], roofline["traffic_source"] = live
            if tr:
                roofline["traffic_committed_profile"] = tr["hbm_bytes_per_launch"]
        elif tr:
            roofline["traffic"] = tr["hbm_bytes_per_launch"]
            roofline["traffic_source"] = tr.get("source")
        if world == 1 and args.batch == 1 and not args.no_live_stats:
            st = live_kernel_stats(n, args.kernel, kernel_used, args.steps, args.warmup, S, args.omega)
            if st:
                roofline.update(st)
                if kernel_used == "matfree_tb":
                    roofline["rocprof_frac"] = flops / (st["rocprof_avg_us"] * 1e-6) / 1e12 / FP64_INSTR_PEAK_T
        if explicit:
            el, ek = explicit
            ea = BYTES_PER_CELL_SWEEP * cells / el / 1e9
            # the contract figure (64 B per cell per sweep) on the explicit operator, same run
            roofline["contract_64B_frac"] = ea / HBM_PEAK_GBS
            roofline["contract_64B_kernel"] = ek
            roofline["contract_64B_launch_us"] = el * 1e6
            roofline["contract_64B_achieved_GBs"] = ea
            roofline["contract_64B_Mcells_iter_per_s"] = cells / el / 1e6
            tre = traffic_of(ek)
            if tre:
                roofline["contract_64B_traffic"] = tre["hbm_bytes_per_launch"]
            if world == 1 and args.batch == 1 and not args.no_live_stats:
                # the same figure from rocprofv3 on this box: one child run on the explicit kernel (3 x 300 sweeps)
                ste = live_kernel_stats(n, "explicit", "explicit", 2, 1, 300, args.omega, keep_as="bench_live_explicit_kernel_stats.csv")
                if ste:
                    roofline["contract_64B_rocprof_avg_us"] = ste["rocprof_avg_us"]
                    roofline["contract_64B_rocprof_min_us"] = ste["rocprof_min_us"]
                    roofline["contract_64B_rocprof_calls"] = ste["rocprof_calls"]
                    roofline["contract_64B_rocprof_frac"] = BYTES_PER_CELL_SWEEP * cells / (ste["rocprof_avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS

        out = {
            "metric": "Mcells*iter/s (Jacobi sweep) at 4096^2" if n == 4096 else f"Mcells*iter/s (Jacobi sweep) at {n}^2",
            "value": world * cells * S * args.steps / elapsed / 1e6,
            "unit": "Mcells*iter/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"{n}x{n} synthetic two-phase image (splitmix64 seed 12345, porosity 0.5), Ds=1e-3 Df=1 "
                            f"CL=0 CR=1, omega={args.omega:.6g}; step = {S} sweeps + 1 Deff evaluation; "
                            f"{args.batch} image(s) per GPU (image index = rank), no inter-GPU communication"
                            + ("; REHEARSAL: the ranks share GPUs (--share-gpu)" if args.share_gpu and world > 1 else ""),
                "kernel": kernel_used,
                "sweeps_per_step": S,
                "sweeps_per_launch": sweeps_per_launch,
            },
            "roofline": roofline,
            "per_rank_ms_per_step": per_rank_ms,
        }
        if plan:
            out["config"]["plan"] = plan
        if omega1_ms:
            out["jacobi_omega_1"] = {"value": cells * S / (omega1_ms * 1e-3) / 1e6, "unit": "Mcells*iter/s",
                                     "sample": f"{S} sweeps with omega = 1 (plain Jacobi, updateX_V1), same image, one GPU"}
        if fma_ms:
            out["contracted_arithmetic"] = {
                "value": cells * S / (fma_ms * 1e-3) / 1e6, "unit": "Mcells*iter/s",
                "sample": f"{S} sweeps with deff_set_tuning('fma', 1): sigma += a*x as fma, final sum as fma "
                          "(7 instead of 11 FP64 instructions per cell); parity: bit-identical to the oracle built "
                          "with -ffp-contract=fast"}
            if kernel_used == "matfree_tb":
                fl = FP64_INSTR_PER_CELL[True] * cells * S / (fma_ms * 1e-3) / 1e12
                out["contracted_arithmetic"]["fp64_instr_frac"] = fl / FP64_INSTR_PEAK_T
        if small:
            out["single_image_1024"] = {"value": small[0], "unit": "Mcells*iter/s", "kernel": small[1], "plan": small[2],
                                        "fp64_instr_frac": FP64_INSTR_PER_CELL[False] * small[0] * 1e6 / 1e12 / FP64_INSTR_PEAK_T,
                                        "sample": "4800 sweeps (best of 3) of ONE 1024x1024 synthetic image (BASELINE config #2's "
                                                  "shape), same physics, one GPU"}
        if mid:
            out["single_image_2048"] = {"value": mid[0], "unit": "Mcells*iter/s", "kernel": mid[1], "plan": mid[2],
                                        "fp64_instr_frac": FP64_INSTR_PER_CELL[False] * mid[0] * 1e6 / 1e12 / FP64_INSTR_PEAK_T,
                                        "sample": "2400 sweeps (best of 3) of ONE 2048x2048 synthetic image, same physics, one GPU"}
        if tol1024:
            out["iters_to_tol_1024"] = tol1024
        if resid:
            out["residual_4096" if n == 4096 else f"residual_{n}"] = resid
        if n == 4096 and not lean:
            # BASELINE.json's metric names iterations-to-tolerance AT 4096^2: 610 s of solving cannot sit inside a bench run
            # that has to finish in minutes, so the figure is CITED from the builder's own run, not timed by the driver
            out["iters_to_tol_4096"] = {"iters": 47200001, "seconds": 610, "deff": 0.006838670769926945, "tol": 1e-6,
                                        "source": "profiles/r04_iterations_to_tolerance_4096.log (tools/measure_tol_4096.py)",
                                        "measured_by": "builder, round 4, final kernels (610 s; 657 s before the dealt tiles, 664 s in round 3); same count and Deff in rounds 1, 2 "
                                                       "and 3 -- NOT timed in this run"}
        if world == 1 and not args.no_cpu_baseline:
            base, K, want = cpu_baseline(n, with_reference_kernel=not args.primary_only)
            out["cpu_baseline"] = base
            if not args.primary_only:
                # the same single-thread oracle at configs #1 / #2's sizes (2 000 / 50 sweeps)
                out["cpu_baseline_128"] = cpu_baseline(128, fixed_sweeps=2000)[0]
                out["cpu_baseline_1024"] = cpu_baseline(1024, fixed_sweeps=50)[0]
            if args.batch != 1:
                print(json.dumps(out), flush=True)
                s.close()
                return
            # parity, where the money is: the SAME K sweeps from the same start (linear guess) on the GPU, on the
            # kernel that was just timed, must give the oracle's field bit for bit (north-star bar: 1e-6 rel L2)
            import numpy as np
            s.init_linear(0.0, 1.0)
            s.sweeps(K, 2.0 / 3.0)
            got = s.get_field()
            rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
            equal = bool(np.array_equal(got, want))
            out["parity_checked"] = equal
            out["parity_sweeps"] = K
            out["parity_rel_l2"] = rel
            out["parity_kernel"] = s.kernel_in_use()
            print(json.dumps(out), flush=True)
            assert equal and rel <= 1e-6, f"GPU field after {K} sweeps differs from the oracle's (rel L2 {rel:.3e})"
        else:
            print(json.dumps(out), flush=True)
    s.close()
    if use_dist:
        barrier()                                  # every rank leaves together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
