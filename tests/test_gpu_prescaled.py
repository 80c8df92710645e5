"""set_tuning("prescaled", 1) on the GPU: the library against the CPU model of the pre-scaled five-FMA sweep
(tests/cpp/prescaled_model.c through prescaled_model.py), np.array_equal throughout -- the arithmetic is defined operation by
operation, so every kernel form that runs it must give the model's bits (the model itself is graded against the oracle at a
tolerance in tests/test_prescaled_model.py).

Shapes are the smallest at which each path of the kernels can go wrong, and every run asserts from the plan that it took the
path it was chosen for:
  2 x 2, 3 x 5            too few rows for a blocked pass: the single-sweep kernel alone
  97 x 41                 odd width: a pad column; one strip
  260 x 70                three strips: the middle one has no wall column (no b' lookup)
  260 x 70, tb_LY 16      several chunks per image: the trimmed ramp groups, chunk seams
  3 x (130 x 23)          a stack: tiles at the top of a mesh in the middle of the array
  260 x 70, tb_ranked     dealt tiles on and off (T = 8)
each for 3 T + 3 sweeps (passes and the single-sweep remainder) at T = 1, 2, 4, 6, 8 and with kernel = "matfree", omega 2/3 and
1, and wall values other than 0 / 1."""
import json
import os
import subprocess

import numpy as np
import pytest

import prescaled_model as pm
from conftest import ROOT

pytestmark = pytest.mark.gpu

EINVAL = -1
OMEGAS = (2.0 / 3.0, 1.0)
FORMS = [1, 2, 4, 6, 8, "matfree"]
PHYS = (1e-3, 1.0, 0.0, 1.0)                            # Ds, Df, CL, CR


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def rand_mask(rng, nx, ny, p=0.5):
    return np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8)


def model_sweeps(oracle, pix, x0, n, omega, phys=PHYS):
    Ds, Df, CL, CR = phys
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, Df, Ds), CL, CR)
    return pm.sweeps(A, b, x0, n, omega)


def run(pkg, pix, x0, n, omega, form, tune=None, nimg=1, phys=PHYS):
    """(field, plan, kernel in use) after ONE sweeps(n) call with the key set."""
    ny, nx = pix.shape[0] // nimg, pix.shape[1]
    with pkg.Solver(nx, ny, nimg=nimg, kernel="matfree" if form == "matfree" else "matfree_tb") as s:
        s.set_tuning("prescaled", 1)
        if form != "matfree":
            s.set_tuning("tb_T", form)
        for k, v in (tune or {}).items():
            s.set_tuning(k, v)
        s.set_image(pix if nimg == 1 else pix.reshape(nimg, ny, nx))
        s.assemble_2phase(*phys)
        s.set_field(x0)
        s.sweeps(n, omega)
        plan = s.plan()
        plan["tb_chain"] = s.plan_value("tb_chain")
        return s.get_field(), plan, s.kernel_in_use()


def sweeps_of(form):
    return 27 if form == "matfree" else 3 * form + 3


def check_blocked(plan, kern, form, strips=1, chunks=1):
    assert plan["prescaled"] == 1, plan
    if form == "matfree":
        assert kern == "matfree"
        return
    assert kern == "matfree_tb"
    assert (plan["tb_T"], plan["tb_impl"], plan["tb_chain"], plan["tb_resident"]) == (form, 1, 0, 0), plan
    assert plan["tb_strips"] >= strips and plan["tb_chunks_per_image"] >= chunks, plan


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 5)])
def test_meshes_too_small_for_a_blocked_pass(pkg, oracle, nx, ny, form):
    rng = np.random.default_rng(nx * 100 + ny)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    for om in OMEGAS:
        got, plan, kern = run(pkg, pix, x0, sweeps_of(form), om, form)
        assert kern == "matfree" and plan["prescaled"] == 1, (kern, plan)
        assert np.array_equal(got, model_sweeps(oracle, pix, x0, sweeps_of(form), om)), om


@pytest.mark.parametrize("form", FORMS)
def test_odd_width_with_a_pad_column(pkg, oracle, form):
    nx, ny = 97, 41
    rng = np.random.default_rng(97)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    for om in OMEGAS:
        for phys in (PHYS, (0.05, 2.5, 0.25, 1.75)):
            got, plan, kern = run(pkg, pix, x0, sweeps_of(form), om, form, phys=phys)
            check_blocked(plan, kern, form)
            assert np.array_equal(got, model_sweeps(oracle, pix, x0, sweeps_of(form), om, phys)), (om, phys)


@pytest.mark.parametrize("form", FORMS)
def test_three_strips_the_middle_one_without_a_wall_column(pkg, oracle, form):
    nx, ny = 260, 70
    rng = np.random.default_rng(260)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    for om in OMEGAS:
        for phys in (PHYS, (0.05, 2.5, 0.25, 1.75)):
            got, plan, kern = run(pkg, pix, x0, sweeps_of(form), om, form, phys=phys)
            check_blocked(plan, kern, form, strips=3)
            assert np.array_equal(got, model_sweeps(oracle, pix, x0, sweeps_of(form), om, phys)), (om, phys)


@pytest.mark.parametrize("form", FORMS[:-1])
def test_several_chunks_and_the_trimmed_ramps(pkg, oracle, form):
    nx, ny = 260, 70
    rng = np.random.default_rng(2600)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    for om in OMEGAS:
        got, plan, kern = run(pkg, pix, x0, sweeps_of(form), om, form, tune={"tb_LY": 16})
        check_blocked(plan, kern, form, strips=3, chunks=2)
        assert plan["tb_LY"] == 16 and plan["tb_ranked"] == 0, plan
        assert np.array_equal(got, model_sweeps(oracle, pix, x0, sweeps_of(form), om)), om


@pytest.mark.parametrize("form", FORMS)
def test_stack_of_three(pkg, oracle, form):
    nx, ny, B = 130, 23, 3
    rng = np.random.default_rng(130)
    pixs = [rand_mask(rng, nx, ny, 0.4 + 0.1 * k) for k in range(B)]
    x0 = rng.random((B * ny, nx))
    for om in OMEGAS:
        got, plan, kern = run(pkg, np.concatenate(pixs), x0, sweeps_of(form), om, form, nimg=B)
        check_blocked(plan, kern, form, strips=2)
        for k in range(B):
            want = model_sweeps(oracle, pixs[k], x0[k * ny:(k + 1) * ny], sweeps_of(form), om)
            assert np.array_equal(got[k * ny:(k + 1) * ny], want), (om, k)


@pytest.mark.parametrize("ranked", [0, 1])
def test_dealt_tiles_on_and_off(pkg, oracle, ranked):
    nx, ny = 260, 70
    rng = np.random.default_rng(70)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    for om in OMEGAS:
        got, plan, kern = run(pkg, pix, x0, 27, om, 8, tune={"tb_ranked": ranked})
        check_blocked(plan, kern, 8, strips=3)
        assert plan["tb_ranked"] == ranked, plan
        assert np.array_equal(got, model_sweeps(oracle, pix, x0, 27, om)), om


# ---- 3-phase dictionaries: harvested from the explicit system, and native (flood fill and row codes on the device)

@pytest.mark.parametrize("native", [False, True])
def test_3phase_dictionaries(pkg, oracle, native):
    nx, ny = 75, 40
    rng = np.random.default_rng(75)
    f = np.kron(rng.random((ny // 4 + 1, nx // 3 + 1)), np.ones((4, 3)))[:ny, :nx]
    pix = np.where(f < 0.5, 0, np.where(f < 0.72, 150, 255)).astype(np.uint8)
    grid, _ = oracle.floodfill((pix > 200).astype(np.uint32))
    assert (grid == 2).any() or (grid == 1).any()
    D = oracle.fill_D_3phase(pix, 1.0, 0.0, 1237500.0)
    with np.errstate(all="ignore"):
        A, b = oracle.discretize(D, 0.0, 1.0, grid=grid)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("prescaled", 1)
        s.set_image(pix)
        if native:
            s.assemble_3phase_native(0.0, 1.0, 1237500.0, 0.0, 1.0)
        else:
            s.assemble_3phase(0.0, 1.0, 1237500.0, 0.0, 1.0, grid)
        s.init_linear(0.0, 1.0)
        s.sweeps(15)
        plan = s.plan()
        assert s.kernel_in_use() == "matfree_tb" and (plan["prescaled"], plan["tb_impl"], plan["tb_T"]) == (1, 1, 4), plan
        got = s.get_field()
    assert np.array_equal(got, pm.sweeps(A, b, x0, 15))


# ---- solves

@pytest.fixture(scope="module")
def config1_model(oracle, img00000):
    D = oracle.fill_D_2phase(img00000, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    return pm.jacobi(A, b, oracle.linear_guess(128, 128, 0.0, 1.0), D, 0.0, 1.0, 1e-6, 500000)


def test_config1_solve(pkg, img00000, config1_model):
    it, deff, conv, x, MFL, MFR = config1_model
    with pkg.Solver(128, 128) as s:
        s.set_tuning("prescaled", 1)
        s.set_image(img00000)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        r = s.solve(1e-6, 500000)
        got = s.get_field()
        assert s.plan()["prescaled"] == 1
    assert r.iters == it == 110001
    assert r.deff_raw == deff and r.conv == conv
    assert np.array_equal(got, x)
    assert np.array_equal(r.MFL, MFL) and np.array_equal(r.MFR, MFR)


def small_images(oracle, n):
    """64^2 images of different porosity (different stopping sweeps), their model solves at check_every 100"""
    out = []
    for k in range(n):
        rng = np.random.default_rng(640 + k)
        pix = rand_mask(rng, 64, 64, 0.35 + 0.2 * k)
        D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
        A, b = oracle.discretize(D, 0.0, 1.0)
        out.append((pix, pm.jacobi(A, b, oracle.linear_guess(64, 64, 0.0, 1.0), D, 0.0, 1.0, 1e-3, 100000, check_every=100)))
    return out


def test_solve_batch_images_stop_at_different_sweeps(pkg, oracle):
    imgs = small_images(oracle, 2)
    assert imgs[0][1][0] != imgs[1][1][0], "the two images must stop at different sweeps"
    with pkg.Solver(64, 64, nimg=2) as s:
        s.set_tuning("prescaled", 1)
        s.set_image(np.stack([p for p, _ in imgs]))
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        rs = s.solve(1e-3, 100000, check_every=100)
        field = s.get_field()
        assert s.plan()["prescaled"] == 1
    for k, (pix, (it, deff, conv, x, MFL, MFR)) in enumerate(imgs):
        with pkg.Solver(64, 64) as s:
            s.set_tuning("prescaled", 1)
            s.set_image(pix)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            r1 = s.solve(1e-3, 100000, check_every=100)
            x1 = s.get_field()
        assert (rs[k].iters, rs[k].deff_raw, rs[k].conv) == (r1.iters, r1.deff_raw, r1.conv) == (it, deff, conv), k
        assert np.array_equal(field[k * 64:(k + 1) * 64], x1) and np.array_equal(x1, x), k
        assert np.array_equal(rs[k].MFL, MFL) and np.array_equal(rs[k].MFR, MFR), k


def test_solve_stream_two_slots_three_images(pkg, oracle):
    imgs = small_images(oracle, 3)
    with pkg.Solver(64, 64, nimg=2) as s:
        s.set_tuning("prescaled", 1)
        rs = s.solve_stream([p for p, _ in imgs], 1e-3, 1.0, 0.0, 1.0, 1e-3, 100000, check_every=100, want_fields=True)
        assert s.plan()["prescaled"] == 1
    assert len(rs) == 3
    for k, (pix, (it, deff, conv, x, _, _)) in enumerate(imgs):
        assert (rs[k].iters, rs[k].deff_raw, rs[k].conv) == (it, deff, conv), k
        assert np.array_equal(rs[k].field, x), k


def test_full_size_4096(pkg, oracle):
    nx = ny = 4096
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    want = pm.sweeps(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), 27)
    del A, b
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("prescaled", 1)
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(27)
        plan = s.plan()
        assert (plan["prescaled"], plan["tb_T"], plan["tb_impl"], s.plan_value("tb_chain")) == (1, 8, 1, 0), plan
        assert plan["tb_strips"] >= 2 and plan["tb_chunks_per_image"] >= 2, plan
        got = s.get_field()
    assert np.array_equal(got, want)


def test_planner_with_the_key_and_back(pkg, oracle):
    nx = ny = 1024
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    want = oracle.sweeps(A, b, x0, 27)
    keys = ("tb_T", "tb_LY", "tb_strips", "tb_chunks_per_image", "tb_blocks", "tb_impl", "tb_R", "tb_NW", "tb_resident", "tb_ranked")
    with pkg.Solver(nx, ny) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(27)
        before = {k: s.plan()[k] for k in keys}
        assert s.plan()["prescaled"] == 0 and np.array_equal(s.get_field(), want)
        s.set_tuning("prescaled", 1)
        s.init_linear(0.0, 1.0)
        s.sweeps(27)
        plan = s.plan()
        assert (plan["prescaled"], plan["tb_impl"], plan["tb_resident"], s.plan_value("tb_chain")) == (1, 1, 0, 0), plan
        assert np.array_equal(s.get_field(), pm.sweeps(A, b, x0, 27))
        s.set_tuning("prescaled", 0)
        s.init_linear(0.0, 1.0)
        s.sweeps(27)
        assert {k: s.plan()[k] for k in keys} == before and s.plan()["prescaled"] == 0, (s.plan(), before)
        assert np.array_equal(s.get_field(), want)


def test_key_switched_on_after_the_table_was_uploaded_and_omega_changed(pkg, oracle):
    """upload_lut returns early on an unchanged omega: the pre-scaled table must still be built, and rebuilt for another omega
    and another dictionary."""
    nx, ny = 97, 41
    rng = np.random.default_rng(4197)
    pix, x0 = rand_mask(rng, nx, ny), rng.random((ny, nx))
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(*PHYS)
        s.set_field(x0)
        s.sweeps(3)                                               # the dictionary's table is on the device for omega 2/3
        s.set_tuning("prescaled", 1)
        for om, phys in ((2.0 / 3.0, PHYS), (1.0, PHYS), (1.0, (0.05, 2.5, 0.25, 1.75)), (2.0 / 3.0, (0.05, 2.5, 0.25, 1.75))):
            s.assemble_2phase(*phys)
            s.set_field(x0)
            s.sweeps(15, om)
            assert s.plan()["prescaled"] == 1
            assert np.array_equal(s.get_field(), model_sweeps(oracle, pix, x0, 15, om, phys)), (om, phys)


# ---- refusals: DEFF_EINVAL at the call that would sweep, the field as it was

def refused(pkg, s, x0):
    with pytest.raises(pkg.DeffError) as e:
        s.sweeps(9)
    assert e.value.code == EINVAL, e.value
    assert np.array_equal(s.get_field(), x0)
    with pytest.raises(pkg.DeffError) as e:
        s.solve(1e-6, 100)
    assert e.value.code == EINVAL, e.value
    assert np.array_equal(s.get_field(), x0)


def test_refused_two_phase_with_a_phase_that_cannot_diffuse(pkg):
    rng = np.random.default_rng(1)
    pix, x0 = rand_mask(rng, 64, 64), rng.random((64, 64))
    with pkg.Solver(64, 64) as s:
        s.set_tuning("prescaled", 1)
        s.set_image(pix)
        s.assemble_2phase(0.0, 1.0, 0.0, 1.0)
        s.set_field(x0)
        refused(pkg, s, x0)


def test_refused_explicit_kernel_and_no_dictionary(pkg, oracle):
    rng = np.random.default_rng(2)
    pix, x0 = rand_mask(rng, 64, 64), rng.random((64, 64))
    with pkg.Solver(64, 64, kernel="explicit") as s:
        s.set_tuning("prescaled", 1)
        s.set_image(pix)
        s.assemble_2phase(*PHYS)
        s.set_field(x0)
        refused(pkg, s, x0)
    # "dict" 0: a system assembled from a D plane gets no row dictionary
    with pkg.Solver(64, 64) as s:
        s.set_tuning("prescaled", 1)
        s.set_tuning("dict", 0)
        s.set_image(pix)
        s.assemble_from_D(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
        s.set_field(x0)
        refused(pkg, s, x0)
        # ... and the same context sweeps once the key is off
        s.set_tuning("prescaled", 0)
        s.sweeps(9)
        A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
        assert np.array_equal(s.get_field(), oracle.sweeps(A, b, x0, 9))


def test_refused_values_and_slabs(pkg):
    with pkg.Solver(64, 64) as s:
        with pytest.raises(pkg.DeffError) as e:
            s.set_tuning("prescaled", 2)
        assert e.value.code == EINVAL
    with pkg.SlabGroup(64, 64, [0, 0]) as g:
        with pytest.raises(pkg.DeffError) as e:
            g.set_tuning("prescaled", 1)
        assert e.value.code == EINVAL


# ---- the command-line driver

def test_driver_arith_prescaled_config1(pkg, config1_model, tmp_path):
    """deff2d --arith prescaled on config #1 (RunBatch 1, one image: the reference's BatchSim of 00000.jpg).  The CSV keeps the
    reference's columns, which have no iteration count: that is read from --json and from the Verbose output."""
    import shutil
    from conftest import GOLDEN
    it, deff, conv, _, _, _ = config1_model
    exe = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
    shutil.copy(os.path.join(GOLDEN, "00000.jpg"), tmp_path / "00000.jpg")
    kv = dict(Phases=2, Ds="1e-3", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0, OutputName="out.csv", printCMap=0,
              Convergence="1e-6", MaxIter="5e5", Verbose=1, RunBatch=1, NumImages=1)
    (tmp_path / "input.txt").write_text("\n".join(["Input File:"] + [f"{k}: {v}" for k, v in kv.items()]) + "\n")
    r = subprocess.run([exe, "input.txt", "--arith", "prescaled", "--json", "res.json"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.load(open(tmp_path / "res.json"))["results"]
    assert len(res) == 1 and res[0]["iterations"] == it == 110001, res
    assert "Iterations taken = 110001" in r.stdout
    assert abs(res[0]["Deff"] - 0.18286248993335824) <= 1e-10 * 0.18286248993335824
    assert res[0]["Deff"] == deff and res[0]["converge"] == conv
    rows = [ln for ln in (tmp_path / "out.csv").read_text().splitlines() if ln.strip()]
    assert len(rows) == 2 and rows[1].split(",")[3] == f"{deff:f}", rows
    # one image over row slabs: refused with a message before anything runs
    kv.update(RunBatch=0, InputName="00000.jpg")
    (tmp_path / "slabs.txt").write_text("\n".join(["Input File:"] + [f"{k}: {v}" for k, v in kv.items()]) + "\n")
    r = subprocess.run([exe, "slabs.txt", "--arith", "prescaled", "--devices", "0,0"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--arith prescaled does not run over row slabs" in r.stderr, r.stderr
