"""loop_ms and the CSV Time column: the one output no other test reads.

deff_result.loop_ms is the hipEvent time between an event recorded when a solve loop starts (ev0) and one recorded when it
ends -- or, in a stream, at the check that retires an image.  The loops may call back into the host between the two
(deff_set_progress, deff_image_done_fn), and the header allows deff_residual / deff_residual_slot inside those callbacks.
A residual that records the loop's own events moves ev0: every later loop_ms then counts from the last residual call,
about one check interval instead of the whole loop, and deff2d's Time column (which calls deff_residual_slot for every image
a stream retires) inherits it.  The residual therefore times itself with its own event pair (api_residual.hip).

No absolute time is asserted.  The bounds follow from the structure of the code:
  * upper: the device window [ev0, ev1] opens and closes inside the call, so loop_ms <= the host wall time of the call;
  * lower: the first callback runs after a synchronisation that follows ev0, the closing event is recorded after the last
    callback, so the host time between the first and the last callback entry lies inside the window.  The factor 1/2
    separates "about the whole span" from "about one twentieth of it" (a solve with 20 checks) or from "about nothing"
    (a stream), and leaves room for the two clock domains to differ; it is not a measured number.
"""
import ctypes as C
import math
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def _timed_solve_with_residual_callback(pkg, oracle, nimg):
    nx = ny = 256
    Cc, checks = 500, 20
    pix = np.stack([oracle.synth_mask(nx, ny, 41, k) for k in range(nimg)])
    stamps, resid = [], []
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_image(pix if nimg > 1 else pix[0])
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(8)                                             # first-launch costs stay outside the timed call
        s.init_linear(0.0, 1.0)

        def cb(k, d, ch):
            stamps.append(time.monotonic())
            resid.append(s.residual())

        s.set_progress(cb)
        t0 = time.monotonic()
        r = s.solve(1e-30, checks * Cc + 1, check_every=Cc)
        wall_ms = (time.monotonic() - t0) * 1e3
        s.set_progress(None)
    res = r if nimg > 1 else [r]
    assert all(q.iters == checks * Cc + 1 and q.checks == checks + 1 for q in res)
    return res, stamps, resid, wall_ms


@pytest.mark.gpu
def test_loop_ms_of_a_solve_whose_progress_callback_takes_the_residual(pkg, oracle):
    """deff_solve, 256^2, 21 checks, s.residual() in every one: loop_ms spans them all."""
    res, stamps, resid, wall_ms = _timed_solve_with_residual_callback(pkg, oracle, 1)
    assert len(stamps) == 21 and all(np.isfinite(resid)) and resid[0] > resid[-1] > 0
    span_ms = (stamps[-1] - stamps[0]) * 1e3
    print(f"loop_ms {res[0].loop_ms:.3f}  callback span {span_ms:.3f} ms  wall {wall_ms:.3f} ms")
    assert span_ms > 0
    assert 0.5 * span_ms <= res[0].loop_ms <= wall_ms, (res[0].loop_ms, span_ms, wall_ms)


@pytest.mark.gpu
def test_loop_ms_of_a_stack_solved_with_the_callback_set(pkg, oracle):
    """The same through deff_solve_batch with B = 3 and the same callback set.  A stack reports no progress today
    (deff_solve_batch calls the observer for one-image contexts only), so no residual is taken inside the loop and the lower
    bound is empty unless callbacks arrive; the images share one loop, and its time obeys the same two bounds."""
    res, stamps, _, wall_ms = _timed_solve_with_residual_callback(pkg, oracle, 3)
    span_ms = (stamps[-1] - stamps[0]) * 1e3 if len(stamps) >= 2 else 0.0
    print(f"loop_ms {res[0].loop_ms:.3f}  callbacks {len(stamps)}  span {span_ms:.3f} ms  wall {wall_ms:.3f} ms")
    assert len({q.loop_ms for q in res}) == 1
    assert 0 < res[0].loop_ms and 0.5 * span_ms <= res[0].loop_ms <= wall_ms, (res[0].loop_ms, span_ms, wall_ms)


@pytest.mark.gpu
def test_loop_ms_along_a_stream_whose_done_callback_takes_the_slot_residual(pkg, oracle):
    """Seven 128^2 images through ONE slot, each to the same max_iter; the done callback calls deff_residual_slot, as deff2d
    does.  loop_ms is the stream's time when the image retired: it never decreases and it spans the callbacks."""
    from effectivediffusivityfvm_amd import _capi
    nx = ny = 128
    n_img, max_iter, Cc = 7, 4001, 1000
    pixs = [oracle.synth_mask(nx, ny, 97, k) for k in range(n_img)]
    order, stamps, loop_ms, resid, errors = [], [], [], {}, []
    with pkg.Solver(nx, ny, nimg=1) as s:
        L, ctx = s._L, s._ctx
        fed = [0]

        def _next(_u, _slot, pix_ptr, id_ptr):
            if fed[0] >= n_img:
                return 0
            a = np.ascontiguousarray(pixs[fed[0]])
            C.memmove(pix_ptr, a.ctypes.data, a.size)
            id_ptr[0] = fed[0]
            fed[0] += 1
            return 1

        def _done(_u, image_id, slot, res_ptr):
            try:
                stamps.append(time.monotonic())
                order.append(int(image_id))
                assert res_ptr[0].iters == max_iter
                loop_ms.append(res_ptr[0].loop_ms)
                r = C.c_double()
                _capi.check(L.deff_residual_slot(ctx, slot, C.byref(r)))
                resid[int(image_id)] = r.value
            except Exception as e:          # noqa: BLE001 - an exception inside a ctypes callback is swallowed
                errors.append(e)

        nxt, dn = _capi.NEXT_IMAGE_FN(_next), _capi.IMAGE_DONE_FN(_done)
        t0 = time.monotonic()
        rc = L.deff_solve_stream(ctx, nx, ny, 1, 1, 1e-3, 1.0, 0.0, 1.0, 2.0 / 3.0, 1e-30, max_iter, Cc, nxt, dn, None)
        wall_ms = (time.monotonic() - t0) * 1e3
    if errors:
        raise errors[0]
    _capi.check(rc)
    assert order == list(range(n_img))                          # one slot: retirement order is input order
    host_ms = (stamps[-1] - stamps[0]) * 1e3
    print("loop_ms", [round(v, 3) for v in loop_ms], f" host first..last {host_ms:.3f} ms  wall {wall_ms:.3f} ms")
    assert all(math.isfinite(v) and v > 0 for v in loop_ms)
    assert all(b >= a for a, b in zip(loop_ms, loop_ms[1:])), loop_ms
    assert loop_ms[-1] - loop_ms[0] >= 0.5 * host_ms, (loop_ms, host_ms)
    assert loop_ms[-1] <= wall_ms, (loop_ms[-1], wall_ms)
    for k, pix in enumerate(pixs):                              # and the residuals are the oracle's
        D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
        A, b = oracle.discretize(D, 0.0, 1.0)
        x = oracle.sweeps(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), max_iter)
        oracle.assert_residual(resid[k], x, D, 0.0, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("plane", [False, True])
def test_the_residuals_own_ms(pkg, oracle, plane):
    """deff_residual / deff_residual_D report the device time of their own reduction: positive, inside the call."""
    nx = ny = 1024
    pix = oracle.synth_mask(nx, ny, 5, 0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3) if plane else None
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(8)
        first = s.residual(D, 0.0, 1.0) if plane else s.residual()
        for _ in range(3):
            t0 = time.monotonic()
            r, ms = s.residual(D, 0.0, 1.0, timing=True) if plane else s.residual(timing=True)
            wall_ms = (time.monotonic() - t0) * 1e3
            print(f"residual ms {ms:.4f}  wall {wall_ms:.4f} ms")
            assert r == first and 0 < ms <= wall_ms, (ms, wall_ms)


@pytest.mark.gpu
def test_driver_time_column_along_one_slot(tmp_path):
    """deff2d, RunBatch 1, six equal images forced through one slot (--batch-size 1), every one to MaxIter: Time is the
    stream's device time when the image retired (deff2d --help), so it grows along the stream -- the last retired image's is
    about six times the first's; a Time that restarts at every retirement would make them about equal."""
    from PIL import Image
    rng = np.random.default_rng(321)
    n_img = 6
    for k in range(n_img):
        a = np.where(rng.random((64, 96)) < 0.4 + 0.02 * k, 0, 255).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / f"{k:05d}.jpg", quality=95)
    lines = ["Input File:"] + [f"{k}: {v}" for k, v in dict(
        Phases=2, Ds="1e-2", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0, OutputName="out.csv", printCMap=0, Convergence="1e-30",
        MaxIter="1e5", Verbose=0, RunBatch=1, NumImages=n_img).items()]
    open(tmp_path / "input.txt", "w").write("\n".join(lines) + "\n")
    t0 = time.monotonic()
    r = subprocess.run([EXE, "input.txt", "--json", "res.json", "--batch-size", "1", "--prefetch-threads", "1", "--progress", "prog.txt"],
                       cwd=tmp_path, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    wall = time.monotonic() - t0
    assert r.returncode == 0, r.stderr + r.stdout
    rows = open(tmp_path / "out.csv").read().splitlines()
    t = rows[0].split(",").index("Time")
    times = [float(row.split(",")[t]) for row in rows[1:]]
    retired = [int(ln.split()[0]) for ln in open(tmp_path / "prog.txt").read().splitlines()]   # one line per image, as they retire
    print("Time", times, "retired", retired, f"wall {wall:.3f} s")
    assert len(times) == n_img and sorted(retired) == list(range(n_img))
    assert all(math.isfinite(v) and 0 <= v <= wall for v in times), (times, wall)
    assert times[retired[-1]] >= 2 * times[retired[0]], (times, retired)
    import json
    assert all(q["iterations"] == 100000 for q in json.load(open(tmp_path / "res.json"))["results"])
