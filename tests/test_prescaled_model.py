"""The pre-scaled five-FMA sweep (set_tuning("prescaled", 1)) as arithmetic, on the CPU: tests/cpp/prescaled_model.c against
the oracle.  No GPU.

The pre-scaled form is NOT the reference's written operation order, so it is graded at a tolerance: field rel-L2 <= 1e-9 and
Deff relative <= 1e-10 on full solves -- three and two orders inside the project's 1e-6 / 1e-8 -- with the SAME sweep counts
(the stopping rule must fire at the same check), and rel-L2 <= 1e-12 after 1 000 sweeps.  Measured when the model was written:
at most 5.6e-13 / 1.1e-12 on full solves, 7.4e-15 after 1 000 sweeps; the oracle's own contracted flavour ("fma") differs
from its default by 1.4e-14 ... 1.1e-12, the same order."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import prescaled_model as pm
from conftest import GOLDEN


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_config1_in_full(oracle, img00000, recorded):
    """00000.jpg, 128^2, Ds 1e-3, tol 1e-6: 110 001 = 110 001 sweeps."""
    rec = recorded["img00000_2phase_batch"]
    want = np.load(os.path.join(GOLDEN, "img00000_field.npy"))            # the oracle's field after its 110 001 sweeps
    D = oracle.fill_D_2phase(img00000, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    want_deff = oracle.flux_deff(want, D, 0.0, 1.0)[0]
    assert want_deff == rec["deff_build_b"]
    it, deff, conv, x, _, _ = pm.jacobi(A, b, oracle.linear_guess(128, 128, 0.0, 1.0), D, 0.0, 1.0, 1e-6, 500000)
    print(f"config #1: {it} sweeps, field rel-L2 {rel_l2(x, want):.2e}, Deff relative {abs(deff - want_deff) / want_deff:.2e}")
    assert it == 110001 == rec["iters"]
    assert np.all(np.isfinite(x))
    assert rel_l2(x, want) <= 1e-9
    assert abs(deff - want_deff) <= 1e-10 * want_deff


def model_solve_3phase(pix, DCS, DCF, DCG, CL, CR, tol, max_iter):
    """oracle_binding.solve_3phase with the model's Jacobi loop."""
    ny, nx = pix.shape
    grid, _ = ob.floodfill((pix > 200).astype(np.uint32))
    x = ob.linear_guess(nx, ny, CL, CR)
    stages = []
    g = 10.0
    while g < DCG:
        D = ob.fill_D_3phase(pix, DCF, DCS, g)
        A, b = ob.discretize(D, CL, CR, grid=grid)
        it, _, _, x, _, _ = pm.jacobi(A, b, x, D, CL, CR, tol * 10, max_iter)
        stages.append(it)
        g = g * 10
    D = ob.fill_D_3phase(pix, DCF, DCS, DCG)
    A, b = ob.discretize(D, CL, CR, grid=grid)
    it, deff, conv, x, _, _ = pm.jacobi(A, b, x, D, CL, CR, tol, max_iter)
    stages.append(it)
    return dict(stage_sweeps=stages, deff=deff / DCF, conv=conv, field=x)


def test_3phase_as_shipped_flow(oracle, img00000, recorded):
    """The reference's shipped configuration on 00000.jpg: Ds 0, Dg 1 237 500, tol 1e-5, flood fill, ImpSolid rows, 7 stages."""
    rec = recorded["img00000_3phase_as_shipped"]
    o = rec["options"]
    with np.errstate(all="ignore"):
        want = oracle.solve_3phase(img00000, o["Ds"], o["Df"], o["Dg"], o["CL"], o["CR"], o["tol"], o["max_iter"])
        got = model_solve_3phase(img00000, o["Ds"], o["Df"], o["Dg"], o["CL"], o["CR"], o["tol"], o["max_iter"])
    print(f"3-phase: stages {got['stage_sweeps']}, field rel-L2 {rel_l2(got['field'], want['field']):.2e}, "
          f"Deff relative {abs(got['deff'] - want['deff']) / want['deff']:.2e}")
    assert want["stage_sweeps"] == rec["stage_sweeps"]
    assert got["stage_sweeps"] == rec["stage_sweeps"] and len(got["stage_sweeps"]) == 7
    assert np.all(np.isfinite(got["field"]))
    assert rel_l2(got["field"], want["field"]) <= 1e-9
    assert abs(got["deff"] - want["deff"]) <= 1e-10 * want["deff"]


@pytest.mark.parametrize("nx,ny", [(97, 41), (64, 64)])
def test_1000_sweeps_and_the_switch_is_real(oracle, nx, ny):
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    got = pm.sweeps(A, b, x0, 1000)
    want = oracle.sweeps(A, b, x0, 1000)
    want_fma = oracle.sweeps(A, b, x0, 1000, flavour="fma")
    print(f"{nx}x{ny}: rel-L2 to the default oracle {rel_l2(got, want):.2e}, to its fma flavour {rel_l2(got, want_fma):.2e}")
    assert rel_l2(got, want) <= 1e-12
    assert not np.array_equal(got, want) and not np.array_equal(got, want_fma)


def test_table_is_one_rounded_product_per_entry(oracle):
    pix = oracle.synth_mask(33, 17, 7, 0)
    D = oracle.fill_D_2phase(pix, 2.5, 0.3)
    A, b = oracle.discretize(D, 0.25, 1.5)
    w = 2.0 / 3.0
    Ap, bp = pm.table(A, b, w)
    c0 = w / A[:, 0]
    assert np.array_equal(Ap, c0[:, None] * A[:, 1:]) and np.array_equal(bp, c0 * b)
