"""deff_solve_cg on the explicit coefficient planes (kernels_cg_planes.hpp, tuning key "cg_planes"): the bits of the table
form wherever a dictionary exists (key 2 against key 0), and -- for systems that cannot have a dictionary -- the direct
solve, a plain CG in long double, the stop paths, the refusals and what the form must leave alone."""
import numpy as np
import pytest

from test_cg_host import K_PARITY, RESTART_CASE, apply_A, block_thomas, decoupled_of, pcg_numpy, rel_l2, residual_np
from test_gpu_cg import (EPS, PARITY_M, RTOL_PARITY, assert_fluxes_of_field, assert_honest, check_against_direct,
                         three_class_image, wall_clusters)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def last_error(pkg):
    return pkg._capi.load().deff_last_error().decode()


def as_list(r):
    return r if isinstance(r, list) else [r]


def bits(r):
    return [(q.iters, q.rel_residual, q.converged, q.deff_raw) for q in as_list(r)]


def run(s, x0, key, **kw):
    """One solve_cg from x0 under cg_planes = key: everything the two forms have to agree on, and the form that ran."""
    s.set_tuning("cg_planes", key)
    s.set_field(x0)
    r = s.solve_cg(**kw)
    assert_fluxes_of_field(s, r)
    flux = [(q.MFL.copy(), q.MFR.copy()) for q in as_list(r)]
    plan = tuple(s.plan_value(k) for k in ("cg_kr", "cg_strips", "cg_items", "cg_restarts"))
    return bits(r), flux, s.get_field(), plan, s.plan_value("cg_impl")


def assert_same_bits(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for (l0, r0), (l1, r1) in zip(a[1], b[1]):
        assert np.array_equal(l0, l1) and np.array_equal(r0, r1)
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3], (a[3], b[3])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Bits of the table form

NATIVE_SHAPES = [(2, 2), (3, 5), (40, 32), (33, 21), (130, 71), (258, 9)]        # DESIGN.md section 9, geometry table
OTHER_SYSTEMS = [(name, nx, ny) for name in ("from_D-4-levels", "sources-inside", "3phase-grid") for nx, ny in ((130, 71), (97, 41))]
STACKS = [(33, 20, 3), (130, 69, 5)]


def dictionary_system(pkg, oracle, name, nx, ny, nimg=1):
    """A context holding one of the systems of test_gpu_cg.py that have a dictionary, and its linear guess."""
    CL, CR = 0.0, 1.0
    s = pkg.Solver(nx, ny, nimg=nimg)
    if name == "native":
        s.set_image(np.stack([oracle.synth_mask(nx, ny, 12345, k) for k in range(nimg)]))
        s.assemble_2phase(1e-3, 1.0, CL, CR)
    else:
        rng = np.random.default_rng(31)
        pix = oracle.synth_mask(nx, ny, 4711, 0)
        if name == "from_D-4-levels":
            left = np.arange(nx) < nx // 2
            D = np.where(pix < 150, np.where(left, 1.0, 7.0), np.where(left, 1e-2, 0.5))
            s.assemble_from_D(D, CL, CR)
        elif name == "sources-inside":
            D = oracle.fill_D_2phase(pix, 1.0, 1e-2)
            A, b = oracle.discretize(D, CL, CR)
            b = b.copy()
            b[::7] += 0.125
            s.set_system(A, b, D, CL, CR)
        else:
            pix = three_class_image(rng, nx, ny)
            grid, _ = pkg.flood_fill((pix > 200).astype(np.uint32))
            s.set_image(pix)
            s.assemble_3phase(0.0, 1.0, 50.0, CL, CR, grid)
    s.init_linear(CL, CR)
    return s, s.get_field()


def both_forms_agree(s, x0, **kw):
    t = run(s, x0, 0, **kw)
    p = run(s, x0, 2, **kw)
    assert (t[4], p[4]) == (1, 3), (t[4], p[4])
    assert_same_bits(t, p)
    return t


def check_bits_of_table_form(s, x0):
    for k in (1, 2, 5, 20):
        for ce in (1, 7, 64):
            t = both_forms_agree(s, x0, rtol=0.0, max_iter=k, check_every=ce)
            assert all(b[0] == k for b in t[0]), t[0]
    ref = None
    for ce in (1, 7, 64):
        t = both_forms_agree(s, x0, rtol=1e-13, max_iter=20000, check_every=ce)
        assert all(b[0] > 0 for b in t[0])
        if ref is None:
            ref = t
        assert_same_bits(ref, t)                                     # and neither depends on check_every
    return ref


@pytest.mark.parametrize("nx,ny", NATIVE_SHAPES)
def test_planes_give_the_bits_of_the_table_form_native(pkg, oracle, nx, ny):
    s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
    with s:
        check_bits_of_table_form(s, x0)


@pytest.mark.parametrize("name,nx,ny", OTHER_SYSTEMS)
def test_planes_give_the_bits_of_the_table_form_systems(pkg, oracle, name, nx, ny):
    s, x0 = dictionary_system(pkg, oracle, name, nx, ny)
    with s:
        check_bits_of_table_form(s, x0)


@pytest.mark.parametrize("nx,ny,B", STACKS)
def test_planes_give_the_bits_of_the_table_form_stacks(pkg, oracle, nx, ny, B):
    s, x0 = dictionary_system(pkg, oracle, "native", nx, ny, nimg=B)
    with s:
        ref = check_bits_of_table_form(s, x0)
        assert s.plan_value("cg_items") % 4 != 0
        assert len({b[0] for b in ref[0]}) > 1                       # the images freeze at different iterations


def test_planes_give_the_bits_of_the_table_form_large(pkg):
    """kr = 3 (2050 x 1537: 17 strips, last item one row)."""
    nx, ny = 2050, 1537
    with pkg.Solver(nx, ny) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        t = both_forms_agree(s, x0, rtol=0.0, max_iter=5)
        assert t[3][:3] == (3, 17, 17 * -(-ny // 3)) and t[0][0][0] == 5


def test_planes_restart_round(pkg, oracle):
    nx, ny, Ds, rtol = RESTART_CASE
    with pkg.Solver(nx, ny) as s:
        s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        s.assemble_2phase(Ds, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        t = both_forms_agree(s, s.get_field(), rtol=rtol)
        assert t[3][3] >= 1, t[3]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. The same small system without its dictionary

@pytest.mark.parametrize("how", ["set_system", "assemble_from_D"])
def test_planes_without_the_dictionary_of_a_small_system(pkg, oracle, how):
    nx, ny = 33, 21
    pix = oracle.synth_mask(nx, ny, 4711, 0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-2)
    A, b = oracle.discretize(D, 0.0, 1.0)

    def assemble(s):
        if how == "set_system":
            s.set_system(A, b, D, 0.0, 1.0)
        else:
            s.assemble_from_D(D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        return s.get_field()

    with pkg.Solver(nx, ny) as s:
        x0 = assemble(s)
        want = run(s, x0, 0, rtol=RTOL_PARITY)
        assert want[4] == 1 and want[0][0][2]
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("dict", 0)
        x0 = assemble(s)
        with pytest.raises(pkg.DeffError) as ei:
            s.solve_cg(rtol=RTOL_PARITY)
        assert ei.value.code == -1 and "no row dictionary" in last_error(pkg)
        assert np.array_equal(s.get_field(), x0)
        got = run(s, x0, 1, rtol=RTOL_PARITY)
        assert got[4] == 3
        assert_same_bits(want, got)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. Systems that cannot have a dictionary

CELL_SYSTEMS = ["uniform-40x32", "uniform-33x21", "uniform-130x71", "uniform-258x9", "log-97x41", "set_system-33x21",
                "grid-97x41", "zero-block-40x32"]


def per_cell_system(pkg, oracle, case, s=None):
    """(context, nx, ny, D, CL, CR, fixed, compare) of a system with its own row in (nearly) every cell."""
    kind, shape = case.split("-")[:-1], case.split("-")[-1]
    kind = "-".join(kind)
    nx, ny = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(1000 * nx + ny)
    CL, CR = 0.0, 1.0
    D = rng.uniform(0.5, 2.0, (ny, nx))
    if kind == "log":
        D = 10.0 ** rng.uniform(-3.0, 0.0, (ny, nx))
    s = pkg.Solver(nx, ny) if s is None else s
    grid = None
    if kind == "set_system":
        A, b = oracle.discretize(D, CL, CR)
        b = b.copy()
        b[::7] += 0.125
        s.set_system(A, b, D, CL, CR)
    elif kind == "grid":
        pix = three_class_image(rng, nx, ny)
        grid, _ = pkg.flood_fill((pix > 200).astype(np.uint32))
        s.assemble_from_D(D, CL, CR, grid=grid)
    else:
        if kind == "zero-block":
            D[8:16, 10:20] = 0.0
        s.assemble_from_D(D, CL, CR)
    s.init_linear(CL, CR)
    return s, nx, ny, D, CL, CR


@pytest.mark.parametrize("case", CELL_SYSTEMS)
def test_planes_on_systems_without_a_dictionary(pkg, oracle, case):
    s, nx, ny, D, CL, CR = per_cell_system(pkg, oracle, case)
    with s:
        x0 = s.get_field()
        A, b = s.get_system()
        assert len(np.unique(np.column_stack([A, b]), axis=0)) > 511
        dec = decoupled_of(A, b)
        fixed = compare = None
        if case.startswith("grid"):
            assert dec.sum() > 0
            wall, isolated = wall_clusters(A, b, nx, ny)
            fixed, compare = isolated, wall
        if case.startswith("zero-block"):
            assert dec.reshape(ny, nx)[8:16, 10:20].all() and dec.sum() == 80
        # key 0: refused, nothing changed
        with pytest.raises(pkg.DeffError) as ei:
            s.solve_cg(rtol=RTOL_PARITY)
        assert ei.value.code == -1 and "no row dictionary" in last_error(pkg)
        assert np.array_equal(s.get_field(), x0)
        # what float64 can certify of b - A x at the solution (test_gpu_cg.py::test_cg_systems_match_direct_solve): the
        # cases here stay a decade below RTOL_PARITY, so that is the tolerance asked for
        xd = block_thomas(A, b, nx, ny, dec if fixed is None else (dec | fixed))
        floor = EPS * np.linalg.norm(apply_A(np.abs(A), np.abs(xd), nx, ny)) / np.linalg.norm(b)
        print(case, f"float64 floor {floor:.3e}")
        assert 10 * floor <= RTOL_PARITY, floor
        # key 1: converges, the same bits whatever check_every and on a second call
        got = [run(s, x0, 1, rtol=RTOL_PARITY, check_every=ce) for ce in (1, 7, 64, 64)]
        assert all(g[4] == 3 for g in got)
        for g in got[1:]:
            assert_same_bits(got[0], g)
        s.set_field(x0)
        r = s.solve_cg(rtol=RTOL_PARITY)
        x = s.get_field()
        print(case, r, "restarts", s.plan_value("cg_restarts"))
        assert r.converged and r.iters > 0, r
        assert bits(r) == got[0][0] and np.array_equal(x, got[0][2])
        assert np.all(x.ravel()[dec] == 0.0)
        assert_honest(r, RTOL_PARITY, A, b, x, nx, ny)
        assert_fluxes_of_field(s, r)
        check_against_direct(pkg, s, r, nx, ny, fixed=fixed, compare=compare, x0=x0, rtol=RTOL_PARITY, xd=xd)
        # one iteration against a plain CG: the field after k iterations against numpy's CG in long double
        t64 = pcg_numpy(A, b, x0, nx, ny, K_PARITY, np.float64)
        tld = pcg_numpy(A, b, x0, nx, ny, K_PARITY, np.longdouble)
        for k in K_PARITY:
            g = rel_l2(t64.fields[k], tld.fields[k])
            s.set_field(x0)
            rk = s.solve_cg(rtol=0.0, max_iter=k)
            xk = s.get_field()
            assert rk.iters == k and not rk.converged and s.plan_value("cg_impl") == 3
            res = residual_np(A, b, xk, nx, ny)
            assert abs(rk.rel_residual - res) <= 1e-9 * res, (rk.rel_residual, res)
            gap = rel_l2(xk, tld.fields[k].astype(np.float64))
            bar = PARITY_M * max(g, 4 * EPS)
            print(f"k-parity {case} k={k}: g(k) {g:.3e}  GPU gap {gap:.3e}  ratio {gap / max(g, 4 * EPS):.2f}")
            assert gap <= bar, (k, gap, g, bar)
            assert np.all(xk.ravel()[dec] == 0.0)
            assert_fluxes_of_field(s, rk)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Stacks of such systems

def test_planes_stack_gives_the_bits_of_single_images(pkg):
    """Three images with their own per-cell D each (uniform 0.5 ... 2, log-uniform over two and over three decades: their
    iteration counts are far apart); 10 items per image, so one workgroup holds waves of two images."""
    nx, ny, B = 33, 20, 3
    rng = np.random.default_rng(8)
    Ds = [rng.uniform(0.5, 2.0, (ny, nx)), 10.0 ** rng.uniform(-2.0, 0.0, (ny, nx)), 10.0 ** rng.uniform(-3.0, 0.0, (ny, nx))]
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(np.concatenate(Ds), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        rs = s.solve_cg(rtol=RTOL_PARITY)
        X = s.get_field()
        assert s.plan_value("cg_impl") == 3 and s.plan_value("cg_items") % 4 != 0
        assert_fluxes_of_field(s, rs)
    assert len({r.iters for r in rs}) == B, [r.iters for r in rs]
    for k in range(B):
        with pkg.Solver(nx, ny) as s1:
            s1.set_tuning("cg_planes", 1)
            s1.assemble_from_D(Ds[k], 0.0, 1.0)
            s1.init_linear(0.0, 1.0)
            r1 = s1.solve_cg(rtol=RTOL_PARITY)
            x1 = s1.get_field()
            assert s1.plan_value("cg_impl") == 3
        assert rs[k].converged and r1.converged
        assert bits(rs[k]) == bits(r1), (k, rs[k], r1)
        assert np.array_equal(X[k * ny:(k + 1) * ny], x1), k


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Refusals under key 1

def test_planes_refusals_leave_the_field_unchanged(pkg, oracle):
    nx, ny = 40, 32
    rng = np.random.default_rng(77)
    D = rng.uniform(0.5, 2.0, (ny, nx))
    A, b = oracle.discretize(D, 0.0, 1.0)
    p = 10 * nx + 7

    def tampered(col, value):
        Ap = A.copy()
        Ap[p, col] = value
        return Ap

    Aw = A.copy()
    Aw[5 * nx, 1] = -0.25                                            # a wall column's W link: explicit-only system
    cases = [(tampered(2, A[p, 2] * (1.0 + 1e-9)), "symmetric"), (tampered(0, 0.0), "admissible"),
             (tampered(0, -1.0), "admissible"), (tampered(0, np.inf), "admissible"), (Aw, "explicit-only")]
    with pkg.Solver(nx, ny) as s:
        with pytest.raises(pkg.DeffError) as ei:
            s.set_tuning("cg_planes", 3)
        assert ei.value.code == -1
        s.set_tuning("cg_planes", 1)
        for Ap, word in cases:
            s.set_system(Ap, b, D, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            x0 = s.get_field()
            with pytest.raises(pkg.DeffError) as ei:
                s.solve_cg(rtol=1e-10)
            assert ei.value.code == -1 and word in last_error(pkg), (word, last_error(pkg))
            assert np.array_equal(s.get_field(), x0)
            # the same context with the consistent system goes through
            s.set_system(A, b, D, 0.0, 1.0)
            s.set_field(x0)
            r = s.solve_cg(rtol=1e-10)
            assert r.converged and s.plan_value("cg_impl") == 3
    # a stack: a non-zero N link in the first row of image 1
    B = 2
    A2, b2, D2 = np.concatenate([A, A]), np.concatenate([b, b]), np.concatenate([D, D])
    Ap = A2.copy()
    Ap[ny * nx + 5, 4] = -0.25
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_tuning("cg_planes", 1)
        s.set_system(Ap, b2, D2, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        with pytest.raises(pkg.DeffError) as ei:
            s.solve_cg(rtol=1e-10)
        assert ei.value.code == -1 and "symmetric" in last_error(pkg)
        assert np.array_equal(s.get_field(), x0)
        s.set_system(A2, b2, D2, 0.0, 1.0)
        s.set_field(x0)
        rs = s.solve_cg(rtol=1e-10)
        assert all(r.converged for r in rs) and s.plan_value("cg_impl") == 3
        assert bits(rs[0]) == bits(rs[1])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Stop paths on planes

def test_planes_stop_paths(pkg, oracle):
    nx, ny = 40, 32
    rng = np.random.default_rng(5)
    D = rng.uniform(0.5, 2.0, (ny, nx))
    D[8:16, 10:20] = 0.0                                             # decoupled cells, written as exact zeros
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        A, b = s.get_system()
        dec = decoupled_of(A, b).reshape(ny, nx)
        # max_iter = 0
        r = s.solve_cg(rtol=1e-10, max_iter=0)
        x = s.get_field()
        assert r.iters == 0 and not r.converged and s.plan_value("cg_impl") == 3 and s.plan_value("cg_restarts") == 0
        assert np.array_equal(x[~dec], x0[~dec]) and np.all(x[dec] == 0.0) and dec.sum() == 80
        res = residual_np(A, b, x, nx, ny)
        assert abs(r.rel_residual - res) <= 1e-9 * res, (r.rel_residual, res)
        assert_fluxes_of_field(s, r)
        # a converged start: 0 iterations, the same bits
        s.set_field(x0)
        r = s.solve_cg(rtol=1e-10)
        x = s.get_field()
        r2 = s.solve_cg(rtol=1e-10)
        assert r.converged and r.iters > 0 and r2.converged and r2.iters == 0
        assert r2.rel_residual == r.rel_residual and r2.deff_raw == r.deff_raw
        assert np.array_equal(s.get_field(), x)
        assert_honest(r2, 1e-10, A, b, x, nx, ny)
        assert_fluxes_of_field(s, r2)
        # without flux vectors
        s.set_field(x0)
        q = s.solve_cg(rtol=1e-10, fluxes=False)
        assert bits(q) == bits(r) and np.array_equal(s.get_field(), x)
        assert np.all(q.MFL == 0.0) and np.all(q.MFR == 0.0)
    # b = 0 (CL = CR = 0) with x = 0: converged at once
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 0.0)
        A, b = s.get_system()
        assert np.all(b == 0.0)
        s.set_field(np.zeros((ny, nx)))
        r = s.solve_cg(rtol=1e-10)
        assert r.converged and r.rel_residual == 0.0 and r.iters == 0 and s.plan_value("cg_impl") == 3
        assert np.all(s.get_field() == 0.0)
        assert_fluxes_of_field(s, r)
    # every row decoupled (D = 0 everywhere: one distinct row, so the dictionary is switched off to get here)
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("dict", 0)
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(np.zeros((ny, nx)), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        A, b = s.get_system()
        assert np.all(decoupled_of(A, b))
        r = s.solve_cg(rtol=1e-10)
        assert r.converged and r.iters == 0 and r.rel_residual == 0.0 and r.deff_raw == 0.0, r
        assert s.plan_value("cg_impl") == 3 and np.all(s.get_field() == 0.0)
        assert_fluxes_of_field(s, r)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. Nothing leaks

def jacobi_run(s, x0):
    s.set_field(x0)
    r = s.solve(1e-7, 2001, check_every=1000)
    return (r.iters, r.deff_raw, r.conv), s.get_field()


def test_planes_leave_a_per_cell_system_alone(pkg, oracle):
    nx, ny = 97, 41
    rng = np.random.default_rng(3)
    D = rng.uniform(0.5, 2.0, (ny, nx))
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, 0.0, 1.0)
        fresh = (s.get_system(), s.kernel_in_use(), jacobi_run(s, x0))
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 1.0)
        s.set_field(x0)
        r = s.solve_cg(rtol=1e-10)
        assert r.converged and s.plan_value("cg_impl") == 3
        x = s.get_field()
        A, b = s.get_system()
        assert np.array_equal(A, fresh[0][0]) and np.array_equal(b, fresh[0][1])
        assert s.kernel_in_use() == fresh[1]
        oracle.assert_residual(s.residual(D, 0.0, 1.0), x, D, 0.0, 1.0)
        got = jacobi_run(s, x0)
        assert got[0] == fresh[2][0] and np.array_equal(got[1], fresh[2][1])


def test_planes_leave_a_native_system_alone(pkg, oracle):
    nx, ny = 97, 41
    pix = oracle.synth_mask(nx, ny, 4242, 0)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)

    def native():
        s = pkg.Solver(nx, ny)
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        return s

    with native() as s:
        fresh = (s.get_system(), s.kernel_in_use(), jacobi_run(s, x0))
    with native() as s:
        fresh_cg = run(s, x0, 0, rtol=1e-10)
    with native() as s:
        p = run(s, x0, 2, rtol=1e-10)
        assert p[4] == 3 and p[0][0][2]
        x = s.get_field()
        A, b = s.get_system()
        assert np.array_equal(A, fresh[0][0]) and np.array_equal(b, fresh[0][1])
        assert s.kernel_in_use() == fresh[1]
        oracle.assert_residual(s.residual(), x, D, 0.0, 1.0)
        got = jacobi_run(s, x0)
        assert got[0] == fresh[2][0] and np.array_equal(got[1], fresh[2][1])
        t = run(s, x0, 0, rtol=1e-10)
        assert t[4] == 1
        assert_same_bits(fresh_cg, t)
        assert_same_bits(t, p)
