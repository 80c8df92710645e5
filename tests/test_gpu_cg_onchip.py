"""deff_solve_cg with the tuning key "cg_onchip" (kernels_cg_image.hpp: one workgroup iterates one image of at most 16 384
cells in a compute unit's registers and LDS) on the GPU: which form a call takes, the recurrence iteration by iteration against
numpy's plain CG, the fixed point against the direct solve, determinism over stacks / check_every / repeated calls, every stop
path, its independence from the Jacobi path, and the driver's --cg-batch."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cg_host import K_PARITY, RESTART_CASE, apply_A, block_thomas, decoupled_of, rel_l2, residual_np
from test_gpu_cg import (DEFF_TOL, EPS, EXE, PARITY_M, RTOL_PARITY, assert_fluxes_of_field, assert_honest, check_against_direct,
                         plain_pcg_trajectories, wall_clusters)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def onchip(pkg, nx, ny, nimg=1, on=1):
    s = pkg.Solver(nx, ny, nimg=nimg)
    s.set_tuning("cg_onchip", on)
    return s


def two_phase(pkg, pix, Ds=1e-3, CL=0.0, CR=1.0, on=1):
    ny, nx = pix.shape
    s = onchip(pkg, nx, ny, on=on)
    s.set_image(pix)
    s.assemble_2phase(Ds, 1.0, CL, CR)
    s.init_linear(CL, CR)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Selection

def test_selection_by_key_and_size(pkg, oracle):
    pix = oracle.synth_mask(128, 128, 12345, 0)
    with two_phase(pkg, pix, on=0) as s:
        assert s.plan_value("cg_impl") == 0 and s.plan()["cg_impl"] == 0
        assert s.solve_cg(rtol=1e-10).converged
        assert s.plan_value("cg_impl") == 1
        s.set_tuning("cg_onchip", 1)
        s.init_linear(0.0, 1.0)
        assert s.solve_cg(rtol=1e-10).converged
        assert s.plan_value("cg_impl") == 2 and s.plan()["cg_impl"] == 2
        s.set_tuning("cg_onchip", 0)                                 # and back: 0 restores the streaming kernels
        s.init_linear(0.0, 1.0)
        assert s.solve_cg(rtol=1e-10).converged
        assert s.plan_value("cg_impl") == 1
    # 130 x 128 = 16 640 cells: not eligible, the key changes nothing
    pix = oracle.synth_mask(130, 128, 12345, 0)
    got = []
    for on in (1, 0):
        with two_phase(pkg, pix, on=on) as s:
            r = s.solve_cg(rtol=1e-10)
            assert r.converged and s.plan_value("cg_impl") == 1
            got.append((r.iters, r.rel_residual, r.deff_raw, s.get_field()))
    assert got[0][:3] == got[1][:3] and np.array_equal(got[0][3], got[1][3])


def test_cg_onchip_takes_zero_or_one(pkg):
    with pkg.Solver(8, 8) as s:
        with pytest.raises(pkg.DeffError):
            s.set_tuning("cg_onchip", 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. Trajectory: the field after k iterations against numpy's plain CG in long double

SHAPES = [(40, 32), (33, 21), (130, 71), (258, 9), (128, 128), (2, 2), (8192, 2), (2, 8192)]
CASES = [(nx, ny, k) for (nx, ny) in SHAPES for k in K_PARITY]


@pytest.mark.parametrize("nx,ny,k", CASES, ids=[f"{nx}x{ny}-k{k}" for nx, ny, k in CASES])
def test_onchip_k_iterations_match_plain_pcg(pkg, oracle, nx, ny, k):
    """The bar of test_gpu_cg.py::test_cg_k_iterations_match_plain_pcg: M * max(g(k), 4 eps), g(k) = numpy's own float64 to
    long double gap after k iterations, M = 100.  The iteration count and the reported residual are asserted wherever numpy's
    own k-th iterate still has a residual above 4 eps -- every case but 2 x 2 from k = 3 on: four unknowns are solved to
    rounding after 3 iterations (numpy's residual is 3e-19 from then on), p.Ap underflows, the iteration breaks down and is
    restarted from a residual of rounding size, so there is no k-th iterate to compare counts with; the field bar holds all
    the same."""
    pix, A, b, x0, f64, fld, g = plain_pcg_trajectories(oracle, nx, ny)
    with two_phase(pkg, pix) as s:
        r = s.solve_cg(rtol=0.0, max_iter=k)
        x = s.get_field()
        assert s.plan_value("cg_impl") == 2
        assert_fluxes_of_field(s, r)
    res = residual_np(A, b, x, nx, ny)
    solved = residual_np(A, b, f64[k], nx, ny) <= 4 * EPS
    assert not solved or ((nx, ny) == (2, 2) and k >= 3)
    if not solved:
        assert r.iters == k and r.converged is False, r
        assert res >= 1e-6 and abs(r.rel_residual - res) <= 1e-9 * res, (r.rel_residual, res)
    gap = rel_l2(x, fld[k])
    bar = PARITY_M * max(g[k], 4 * EPS)
    print(f"on-chip k-parity {nx}x{ny} k={k}: g(k) {g[k]:.3e}  GPU gap {gap:.3e}  ratio {gap / max(g[k], 4 * EPS):.2f}  "
          f"iterations {r.iters}")
    assert gap <= bar, (gap, g[k], bar)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. Fixed point

def test_onchip_config1_matches_direct_solve(pkg, img00000):
    ny, nx = img00000.shape
    with two_phase(pkg, img00000) as s:
        r = s.solve_cg(rtol=RTOL_PARITY, max_iter=100000)
        assert s.plan_value("cg_impl") == 2
        assert r.converged and r.rel_residual <= RTOL_PARITY and r.iters > 0, r
        A, b = s.get_system()
        assert_honest(r, RTOL_PARITY, A, b, s.get_field(), nx, ny)
        assert_fluxes_of_field(s, r)
        print(r)
        check_against_direct(pkg, s, r, nx, ny)


def test_onchip_three_phase_as_shipped(pkg, img00000):
    ny, nx = img00000.shape
    grid, _ = pkg.flood_fill((img00000 > 200).astype(np.uint32))
    with onchip(pkg, nx, ny) as s:
        s.set_image(img00000)
        s.assemble_3phase(0.0, 1.0, 1237500.0, 0.0, 1.0, grid)
        s.init_linear(0.0, 1.0)
        r = s.solve_cg(rtol=RTOL_PARITY, max_iter=1000000)
        print(r)
        assert s.plan_value("cg_impl") == 2
        assert r.converged, r
        A, b = s.get_system()
        assert decoupled_of(A, b).sum() > 0
        assert_honest(r, RTOL_PARITY, A, b, s.get_field(), nx, ny)
        assert_fluxes_of_field(s, r)
        wall, isolated = wall_clusters(A, b, nx, ny)
        check_against_direct(pkg, s, r, nx, ny, fixed=isolated, compare=wall)


def test_onchip_two_phase_ds0(pkg, img00000):
    ny, nx = img00000.shape
    with two_phase(pkg, img00000, Ds=0.0) as s:
        r = s.solve_cg(rtol=RTOL_PARITY, max_iter=100000)
        print(r)
        assert s.plan_value("cg_impl") == 2
        assert r.converged, r
        A, b = s.get_system()
        assert_honest(r, RTOL_PARITY, A, b, s.get_field(), nx, ny)
        assert_fluxes_of_field(s, r)
        wall, isolated = wall_clusters(A, b, nx, ny)
        assert isolated.sum() > 0
        check_against_direct(pkg, s, r, nx, ny, fixed=isolated, compare=wall)


def test_onchip_assemble_from_D(pkg, oracle):
    """A caller's D plane of four levels (test_gpu_cg.py, "from_D-4-levels"), odd pitch: the harvested dictionary."""
    nx, ny = 97, 41
    pix = oracle.synth_mask(nx, ny, 4711, 0)
    left = np.arange(nx) < nx // 2
    D = np.where(pix < 150, np.where(left, 1.0, 7.0), np.where(left, 1e-2, 0.5))
    with onchip(pkg, nx, ny) as s:
        s.assemble_from_D(D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        A, b = s.get_system()
        dec = decoupled_of(A, b)
        xd = block_thomas(A, b, nx, ny, dec)
        floor = EPS * np.linalg.norm(apply_A(np.abs(A), np.abs(xd), nx, ny)) / np.linalg.norm(b)
        rtol = max(RTOL_PARITY, 10 * floor)
        r = s.solve_cg(rtol=rtol, max_iter=1000000)
        print(r, f"float64 floor {floor:.3e}, rtol {rtol:.3e}")
        assert s.plan_value("cg_impl") == 2
        assert r.converged, r
        assert_honest(r, rtol, A, b, s.get_field(), nx, ny)
        assert_fluxes_of_field(s, r)
        check_against_direct(pkg, s, r, nx, ny, x0=x0, rtol=rtol, xd=xd)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Determinism and state hand-over

def stack_run(pkg, n, B, check_every):
    with onchip(pkg, n, n, nimg=B) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        rs = s.solve_cg(rtol=1e-10, check_every=check_every)
        assert s.plan_value("cg_impl") == 2
        assert_fluxes_of_field(s, rs)
        return [(r.iters, r.rel_residual, r.deff_raw, r.converged) for r in rs], s.get_field()


@pytest.mark.parametrize("B", [3, 300])
def test_onchip_stack_bits(pkg, B):
    """300 images are more than the chip has compute units: workgroups take several.  Every image of the stack gives the bits
    of a one-image on-chip context, whatever check_every (the state is saved and reloaded between launches), and again on a
    fresh context."""
    n = 96
    rs0, X0 = stack_run(pkg, n, B, 64)
    assert all(r[3] for r in rs0) and len({r[0] for r in rs0}) > 1
    for ce in (1, 7, 1000, 64):
        rs, X = stack_run(pkg, n, B, ce)
        assert rs == rs0, ce
        assert np.array_equal(X, X0), ce
    with onchip(pkg, n, n) as s1:
        for k in range(B):
            s1.synth_image(12345, k)
            s1.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s1.init_linear(0.0, 1.0)
            r1 = s1.solve_cg(rtol=1e-10)
            assert s1.plan_value("cg_impl") == 2
            assert (r1.iters, r1.rel_residual, r1.deff_raw, r1.converged) == rs0[k], (k, r1, rs0[k])
            assert np.array_equal(s1.get_field(), X0[k * n:(k + 1) * n]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Stop paths

def test_onchip_max_iter_zero(pkg, oracle):
    pix = oracle.synth_mask(40, 32, 12345, 0)
    for Ds in (1e-3, 0.0):
        with two_phase(pkg, pix, Ds=Ds) as s:
            x0 = s.get_field()
            A, b = s.get_system()
            r = s.solve_cg(rtol=1e-10, max_iter=0)
            x = s.get_field()
            dec = decoupled_of(A, b).reshape(32, 40)
            assert s.plan_value("cg_impl") == 2 and s.plan_value("cg_restarts") == 0
            assert r.iters == 0 and not r.converged
            assert np.array_equal(x[~dec], x0[~dec]) and np.all(x[dec] == 0.0)
            res = residual_np(A, b, x, 40, 32)
            assert abs(r.rel_residual - res) <= 1e-9 * res
            assert_fluxes_of_field(s, r)


def test_onchip_rtol_zero_returns_at_max_iter(pkg, oracle):
    with two_phase(pkg, oracle.synth_mask(40, 32, 12345, 0)) as s:
        r = s.solve_cg(rtol=0.0, max_iter=50, check_every=7)
        x = s.get_field()
        A, b = s.get_system()
        res = residual_np(A, b, x, 40, 32)
        assert s.plan_value("cg_impl") == 2
        assert r.iters == 50 and not r.converged and np.all(np.isfinite(x))
        assert res > 0 and abs(r.rel_residual - res) <= 1e-9 * res, (r.rel_residual, res)
        assert_fluxes_of_field(s, r)


def test_onchip_zero_right_hand_side(pkg, oracle):
    nx, ny = 40, 32
    with two_phase(pkg, oracle.synth_mask(nx, ny, 12345, 0), CL=0.0, CR=0.0) as s:
        A, b = s.get_system()
        assert np.all(b == 0.0)
        s.set_field(np.zeros((ny, nx)))
        r = s.solve_cg(rtol=1e-10)
        assert s.plan_value("cg_impl") == 2
        assert r.converged and r.rel_residual == 0.0 and r.iters == 0
        assert np.all(s.get_field() == 0.0)
        assert_fluxes_of_field(s, r)
        x0 = np.random.default_rng(5).random((ny, nx))
        s.set_field(x0)
        r = s.solve_cg(rtol=1e-10, max_iter=12)
        x = s.get_field()
        assert s.plan_value("cg_impl") == 2
        assert r.iters == 12 and not r.converged and r.rel_residual == np.inf, r
        assert np.all(np.isfinite(x))
        assert float(np.sum(x * apply_A(A, x, nx, ny))) < float(np.sum(x0 * apply_A(A, x0, nx, ny)))
        assert_fluxes_of_field(s, r)


def test_onchip_all_rows_decoupled(pkg):
    nx, ny = 40, 32
    with two_phase(pkg, np.full((ny, nx), 255, dtype=np.uint8), Ds=0.0) as s:
        A, b = s.get_system()
        assert np.all(decoupled_of(A, b))
        r = s.solve_cg(rtol=1e-10)
        assert s.plan_value("cg_impl") == 2
        assert r.converged and r.iters == 0 and r.rel_residual == 0.0 and r.deff_raw == 0.0, r
        assert np.all(s.get_field() == 0.0)
        assert_fluxes_of_field(s, r)


def test_onchip_restart_rounds(pkg, oracle):
    nx, ny, Ds, rtol = RESTART_CASE
    with two_phase(pkg, oracle.synth_mask(nx, ny, 12345, 0), Ds=Ds) as s:
        r = s.solve_cg(rtol=rtol)
        x = s.get_field()
        A, b = s.get_system()
        res = residual_np(A, b, x, nx, ny)
        rounds = s.plan_value("cg_restarts")
        print(r, "restart rounds", rounds, "numpy residual", res)
        assert s.plan_value("cg_impl") == 2
        assert rounds >= 1
        assert r.converged, r
        assert res <= 2 * rtol, (res, rtol)
        assert_honest(r, rtol, A, b, x, nx, ny)
        assert_fluxes_of_field(s, r)


def test_onchip_stack_with_an_image_done_at_the_start(pkg, oracle):
    """Image 1 of 3 is all fluid and starts from its exact solution (test_gpu_cg.py): frozen before the first iteration, its
    field is not touched; its neighbours give the bits of one-image contexts."""
    nx, ny = 33, 20
    pixs = [oracle.synth_mask(nx, ny, 12345, 0), np.zeros((ny, nx), dtype=np.uint8), oracle.synth_mask(nx, ny, 12345, 2)]
    ramp = np.tile((np.arange(nx) + 0.5) / nx, (ny, 1))
    with onchip(pkg, nx, ny, nimg=3) as s:
        s.set_image(np.stack(pixs))
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        X0 = s.get_field()
        X0[ny:2 * ny] = ramp
        s.set_field(X0)
        rs = s.solve_cg(rtol=1e-12)
        X = s.get_field()
        assert s.plan_value("cg_impl") == 2
        assert_fluxes_of_field(s, rs)
    assert rs[1].iters == 0 and rs[1].converged and rs[0].iters > 0 and rs[2].iters > 0
    assert np.array_equal(X[ny:2 * ny], X0[ny:2 * ny])
    for k in (0, 2):
        with two_phase(pkg, pixs[k]) as s1:
            r1 = s1.solve_cg(rtol=1e-12)
            assert rs[k].converged and r1.converged
            assert (rs[k].iters, rs[k].deff_raw, rs[k].rel_residual) == (r1.iters, r1.deff_raw, r1.rel_residual)
            assert np.array_equal(X[k * ny:(k + 1) * ny], s1.get_field()), k


def test_onchip_second_call_from_the_converged_field(pkg, oracle):
    with two_phase(pkg, oracle.synth_mask(40, 32, 12345, 0)) as s:
        r = s.solve_cg(rtol=1e-10)
        x = s.get_field()
        r2 = s.solve_cg(rtol=1e-10)
        assert s.plan_value("cg_impl") == 2
        assert r.converged and r.iters > 0 and r2.converged and r2.iters == 0
        assert r2.rel_residual == r.rel_residual and r2.deff_raw == r.deff_raw
        assert np.array_equal(s.get_field(), x)
        assert_fluxes_of_field(s, r2)


def test_onchip_refusals_leave_the_field_unchanged(pkg, oracle):
    nx, ny = 40, 32
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    Ap = A.copy()
    p = 10 * nx + 7
    Ap[p, 2] = Ap[p, 2] * (1.0 + 1e-9)
    with onchip(pkg, nx, ny) as s:
        s.set_system(Ap, b, D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        with pytest.raises(pkg.DeffError) as ei:
            s.solve_cg(rtol=1e-10)
        assert ei.value.code == -1 and "symmetric" in pkg._capi.load().deff_last_error().decode()
        assert np.array_equal(s.get_field(), x0)
        s.set_system(A, b, D, 0.0, 1.0)                              # a harvested dictionary, partner-consistent
        s.set_field(x0)
        r = s.solve_cg(rtol=1e-10)
        assert r.converged and s.plan_value("cg_impl") == 2
        assert_honest(r, 1e-10, A, b, s.get_field(), nx, ny)
    with pkg.SlabRank(nx, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(pix)
        sr.set_tuning("cg_onchip", 1)
        sr.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        sr.init_linear(0.0, 1.0)
        x0 = sr.get_field()
        L = pkg._capi.load()
        out = (pkg._capi.CGResultC * 1)()
        assert L.deff_solve_cg(sr._ctx, 1e-10, 1000, 64, out, None, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. No leak into the Jacobi path

def test_onchip_cg_does_not_leak_into_jacobi(pkg, oracle):
    nx, ny = 64, 48
    pix = oracle.synth_mask(nx, ny, 4242, 0)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    it, deff, conv, want, _, _ = oracle.jacobi(A, b, x0, D, 0.0, 1.0, 1e-7, 20001, check_every=1000)
    with two_phase(pkg, pix) as s:
        s.set_field(x0)
        rc = s.solve_cg(rtol=1e-10)
        assert rc.converged and s.plan_value("cg_impl") == 2
        s.set_field(x0)
        r = s.solve(1e-7, 20001, check_every=1000)
        x = s.get_field()
    with two_phase(pkg, pix, on=0) as s:
        s.set_field(x0)
        r2 = s.solve(1e-7, 20001, check_every=1000)
        x2 = s.get_field()
    assert (r.iters, r.deff_raw, r.conv) == (r2.iters, r2.deff_raw, r2.conv)
    assert np.array_equal(x, x2)
    assert r.iters == it and abs(r.deff_raw - deff) <= 1e-8 * abs(deff) and np.array_equal(x, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. Driver

def test_deff2d_cg_batch(tmp_path):
    """20 numbered JPEGs, mostly 128 x 128 with a 64 x 64 and a 160 x 160 one (not eligible: the library falls back) in the
    middle, with and without --cg-batch 8: the same rows in the same order, all converged, Deff within 2 DEFF_TOL (each run is
    within DEFF_TOL of the exact value at this rtol: item 3 above)."""
    from PIL import Image
    from test_frontend import _write_input
    rng = np.random.default_rng(20)
    sizes = [128] * 20
    sizes[9], sizes[10] = 64, 160
    for k, n in enumerate(sizes):
        a = rng.random((n // 8, n // 8)) < 0.35                      # blobs of 8 x 8 pixels: survives JPEG's quantisation
        Image.fromarray(np.kron(np.where(a, 255, 0), np.ones((8, 8))).astype(np.uint8), "L").save(tmp_path / f"{k:05d}.jpg", quality=95)
    _write_input(tmp_path / "input.txt", Phases=2, Ds="1e-3", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0, OutputName="out.csv",
                 printCMap=0, Convergence="1e-6", MaxIter="5e5", Verbose=0, RunBatch=1, NumImages=20)
    runs = []
    for extra in ([], ["--cg-batch", "8"]):
        out = f"res{len(extra)}.json"
        r = subprocess.run([EXE, "input.txt", "--json", out, "--solver", "cg", "--cg-rtol", "1e-13"] + extra, cwd=tmp_path,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        runs.append(json.load(open(tmp_path / out))["results"])
    plain, batched = runs
    assert len(plain) == 20 and [q["image"] for q in plain] == [q["image"] for q in batched]
    for a, bq in zip(plain, batched):
        assert a["converge"] <= 1e-13 and bq["converge"] <= 1e-13, (a, bq)
        assert a["iterations"] > 0 and bq["iterations"] > 0
        print(a["image"], a["Deff"], bq["Deff"], abs(a["Deff"] - bq["Deff"]) / abs(a["Deff"]))
        assert abs(a["Deff"] - bq["Deff"]) <= 2 * DEFF_TOL * abs(a["Deff"]), (a, bq)
    rows = open(tmp_path / "out.csv").read().splitlines()
    assert len(rows) == 2 * 21                                       # the CSV is appended to: header + 20 rows per run
