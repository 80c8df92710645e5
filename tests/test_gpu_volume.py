"""Volumes on the GPU (deff_volume_*, kernels_cg_volume.hpp): the assembly bit for bit against the numpy model of fvm_row3
(volume_model.py), a volume of one slice against the 2-D plane form, the iteration against the model's CG in long double, the
fixed point against a dense solve, the stop paths and refusals, and that a Volume leaves a 2-D Solver alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import volume_model as vm
from test_cg_host import rel_l2
from test_gpu_cg import DEFF_TOL, EPS, FIELD_TOL, PARITY_M         # the bars of the same checks on images

pytestmark = pytest.mark.gpu

CL, CR = 0.25, 1.5
EINVAL, ESTATE = -1, -5
RES_BAR = 1e-9                 # rel_residual of a field that is not converged against numpy's float64 evaluation, relative
RES_BAR_CONVERGED = 1e-3       # ... of a converged one against the long-double evaluation (the float64 one is rounding there)


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def last_error(pkg):
    return pkg._capi.load().deff_last_error().decode()


@functools.lru_cache(maxsize=None)
def case(nx, ny, nz):
    """(D, A, b) of the seeded volume: D in [1e-3, 2] with 10 % zeros, the model's rows.  Computed once, never written."""
    D = vm.seeded_D(nx, ny, nz)
    A, b = vm.rows3(D, CL, CR)
    for a in (D, A, b):
        a.setflags(write=False)
    return D, A, b


def bits(r):
    return (r.iters, r.rel_residual, r.converged, r.deff_raw)


def assembled(pkg, nx, ny, nz):
    v = pkg.Volume(nx, ny, nz)
    v.assemble_from_D(case(nx, ny, nz)[0], CL, CR)
    v.init_linear(CL, CR)
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Assembly, bit for bit against the model

ASSEMBLY_SHAPES = [(2, 2, 1), (2, 2, 2),            # smallest meshes
                   (9, 7, 3),                       # odd width, pad column
                   (129, 4, 3), (130, 5, 4),        # a second strip of 1 and 2 columns
                   (16, 3, 5),                      # items of 2 rows straddling slice borders
                   (4, 5, 3000),                    # 15 000 rows, ny does not divide the rows of an item
                   (2, 5, 5000)]                    # 25 000 rows: the planner takes 3 rows per item, ny = 5 does not divide


@pytest.mark.parametrize("nx,ny,nz", ASSEMBLY_SHAPES)
def test_assembly_gives_the_models_bits(pkg, nx, ny, nz):
    D, A, b = case(nx, ny, nz)
    with pkg.Volume(nx, ny, nz) as v:
        assert v.mesh() == (nx, ny, nz, 1.0 / nx, 1.0 / ny, 1.0 / nz)
        v.assemble_from_D(D, CL, CR)
        Ag, bg = v.get_system()
        for k, name in enumerate(("a0", "aW", "aE", "aS", "aN", "aB", "aF")):
            assert np.array_equal(Ag[:, k], A[:, k]) and vm.same_bits(Ag[:, k], A[:, k]), name
        assert np.array_equal(bg, b) and vm.same_bits(bg, b)
        if nz >= 3000:
            # the planner's rows per item on the tall image of ny * nz rows (cg_rows_per_item: strips * rows / 8192, at
            # least 2), and two iterations through items that straddle slice borders at every offset
            v.init_linear(CL, CR)
            x0 = v.get_field()
            r = v.solve_cg(rtol=0.0, max_iter=2)
            assert v.plan_value("cg_kr") == max(2, ny * nz // 8192) and v.plan_value("cg_impl") == 5
            if (nx, ny, nz) == (2, 5, 5000):
                assert v.plan_value("cg_kr") == 3
            assert v.plan_value("cg_items") == -(-ny * nz // v.plan_value("cg_kr"))
            f64, _ = vm.pcg(A, b, x0, D.shape, 2, np.float64)
            fld, _ = vm.pcg(A, b, x0, D.shape, 2, np.longdouble)
            g = rel_l2(f64[2], fld[2])
            gap = rel_l2(v.get_field(), fld[2].astype(np.float64))
            print(f"({nx},{ny},{nz}) kr {v.plan_value('cg_kr')}: g(2) {g:.3e}  GPU gap {gap:.3e}")
            assert r.iters == 2 and gap <= PARITY_M * max(g, 4 * EPS), (gap, g)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. A volume of one slice is the 2-D plane form

@pytest.mark.parametrize("nx,ny", [(9, 7), (130, 33), (258, 9)])
def test_one_slice_is_the_2d_plane_form(pkg, nx, ny):
    D = case(nx, ny, 1)[0]
    with pkg.Solver(nx, ny) as s, pkg.Volume(nx, ny, 1) as v:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D[0], CL, CR)
        v.assemble_from_D(D, CL, CR)
        A2, b2 = s.get_system()
        A3, b3 = v.get_system()
        assert vm.same_bits(A3[:, :5], A2) and vm.same_bits(b3, b2) and np.all(A3[:, 5:] == 0.0)
        s.init_linear(CL, CR)
        v.init_linear(CL, CR)
        assert np.array_equal(v.get_field()[0], s.get_field())
        for kw in (dict(rtol=0.0, max_iter=3), dict(rtol=1e-10)):
            r2 = s.solve_cg(**kw)
            r3 = v.solve_cg(**kw)
            print(nx, ny, kw, r2, r3, "2-D form", s.plan_value("cg_impl"))
            assert bits(r3) == bits(r2), (r3, r2)
            assert vm.same_bits(v.get_field()[0], s.get_field())
            assert np.array_equal(r3.MFL, r2.MFL) and np.array_equal(r3.MFR, r2.MFR)
            assert v.plan_value("cg_impl") == 5
            for key in ("cg_kr", "cg_items", "cg_restarts"):
                assert v.plan_value(key) == s.plan_value(key), key
        assert r3.converged and r3.iters > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. The iteration against the model's CG in long double (the bar and growth function of
#    test_gpu_cg_planes.py::test_planes_on_systems_without_a_dictionary: PARITY_M * max(g(k), 4 eps), g(k) = what float64
#    costs numpy's own CG after k iterations)

K_ITER = tuple(range(1, 11))


@pytest.mark.parametrize("nx,ny,nz", [(9, 7, 3), (130, 5, 4), (16, 3, 5)])
def test_iterations_follow_the_models_cg(pkg, nx, ny, nz):
    D, A, b = case(nx, ny, nz)
    dec = vm.decoupled3(A, b).reshape(D.shape)
    assert dec.any()
    with assembled(pkg, nx, ny, nz) as v:
        x0 = v.get_field()
        f64, _ = vm.pcg(A, b, x0, D.shape, K_ITER, np.float64)
        fld, _ = vm.pcg(A, b, x0, D.shape, K_ITER, np.longdouble)
        for k in K_ITER:
            g = rel_l2(f64[k], fld[k])
            v.set_field(x0)
            rk = v.solve_cg(rtol=0.0, max_iter=k)
            xk = v.get_field()
            assert rk.iters == k and not rk.converged and v.plan_value("cg_impl") == 5
            res = vm.residual3(A, b, xk, D.shape)
            assert abs(rk.rel_residual - res) <= RES_BAR * res, (rk.rel_residual, res)
            gap = rel_l2(xk, fld[k].astype(np.float64))
            bar = PARITY_M * max(g, 4 * EPS)
            print(f"k-parity ({nx},{ny},{nz}) k={k}: g(k) {g:.3e}  GPU gap {gap:.3e}  ratio {gap / max(g, 4 * EPS):.2f}")
            assert gap <= bar, (k, gap, g, bar)
            assert np.all(xk[dec] == 0.0)
            d, MFL, MFR = v.flux()
            assert rk.deff_raw == d and np.array_equal(rk.MFL, MFL) and np.array_equal(rk.MFR, MFR)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. The fixed point against a dense solve of get_system's matrix (the bars of test_gpu_cg.py::check_against_direct with a
#    reference CG: max(1e-10, 10 d_ref), d_ref = where numpy's float64 CG from the same guess to the same rtol lands)

@pytest.mark.parametrize("nx,ny,nz", [(9, 7, 3), (12, 10, 6), (33, 5, 4)])
def test_fixed_point_is_the_dense_solve(pkg, nx, ny, nz):
    rtol = 1e-13
    D = case(nx, ny, nz)[0]
    shape = D.shape
    with assembled(pkg, nx, ny, nz) as v:
        x0 = v.get_field()
        A, b = v.get_system()
        dec = vm.decoupled3(A, b)
        M = vm.dense3(A, shape)[np.ix_(~dec, ~dec)]
        xd = np.zeros(dec.size)
        xd[~dec] = np.linalg.solve(M, b[~dec])
        r = v.solve_cg(rtol=rtol)
        x = v.get_field()
        assert r.converged and r.rel_residual <= rtol and r.iters > 0 and v.plan_value("cg_impl") == 5, r
        assert np.all(x.ravel()[dec] == 0.0) and np.all(np.isfinite(x))
        # rel_residual is the returned field's, recomputed on the host in long double
        res = vm.residual3(A, b, x, shape, np.longdouble)
        assert abs(r.rel_residual - res) <= RES_BAR_CONVERGED * res, (r.rel_residual, res)
        fields, k = vm.pcg(A, b, x0, shape, 1_000_000, np.float64, rtol=rtol)
        sel = ~dec
        d_ref = rel_l2(fields[k].ravel()[sel], xd[sel])
        d_gpu = rel_l2(x.ravel()[sel], xd[sel])
        v.set_field(fields[k])
        deff_np = v.flux()[0]
        v.set_field(xd)
        d_exact = v.flux()[0]
        deff_ref = abs(deff_np - d_exact) / abs(d_exact)
        print(f"({nx},{ny},{nz}) numpy CG: {k} iterations, d_ref {d_ref:.3e}, Deff {deff_ref:.3e}; GPU: {r.iters} iterations, "
              f"field {d_gpu:.3e}, Deff {abs(r.deff_raw - d_exact) / abs(d_exact):.3e}, restarts {v.plan_value('cg_restarts')}")
        assert d_gpu <= max(FIELD_TOL, 10 * d_ref), (d_gpu, d_ref)
        assert abs(r.deff_raw - d_exact) <= max(DEFF_TOL, 10 * deff_ref) * abs(d_exact), (r.deff_raw, d_exact, deff_ref)
        assert abs(d_exact - vm.deff_of(xd.reshape(shape), D, CL, CR)) <= 64 * EPS * abs(d_exact)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Stopping and refusals

def test_stop_paths(pkg):
    nx, ny, nz = 16, 3, 5
    D, A, b = case(nx, ny, nz)
    dec = vm.decoupled3(A, b).reshape(D.shape)
    with assembled(pkg, nx, ny, nz) as v:
        x0 = v.get_field()
        # max_iter = 0
        r = v.solve_cg(rtol=1e-10, max_iter=0)
        x = v.get_field()
        assert r.iters == 0 and not r.converged and v.plan_value("cg_impl") == 5 and v.plan_value("cg_restarts") == 0
        assert np.array_equal(x[~dec], x0[~dec]) and np.all(x[dec] == 0.0) and dec.sum() > 0
        res = vm.residual3(A, b, x, D.shape)
        assert abs(r.rel_residual - res) <= RES_BAR * res, (r.rel_residual, res)
        # rtol = 0: the stop test never holds, max_iter ends the call
        v.set_field(x0)
        r = v.solve_cg(rtol=0.0, max_iter=4)
        assert r.iters == 4 and not r.converged and np.isfinite(r.rel_residual)
        # check_every does not change a bit
        runs = []
        for ce in (1, 7, 1000):
            v.set_field(x0)
            q = v.solve_cg(rtol=1e-10, check_every=ce)
            runs.append((bits(q), v.get_field(), q.MFL.copy(), q.MFR.copy(), v.plan_value("cg_restarts")))
        assert runs[0][0][2] and runs[0][0][0] > 0
        for t in runs[1:]:
            assert t[0] == runs[0][0] and t[4] == runs[0][4]
            assert vm.same_bits(t[1], runs[0][1]) and np.array_equal(t[2], runs[0][2]) and np.array_equal(t[3], runs[0][3])
        # a converged start: 0 iterations, the same bits
        x = v.get_field()
        r2 = v.solve_cg(rtol=1e-10)
        assert r2.converged and r2.iters == 0
        assert r2.rel_residual == runs[-1][0][1] and r2.deff_raw == runs[-1][0][3]
        assert vm.same_bits(v.get_field(), x)
        # without flux vectors
        v.set_field(x0)
        q = v.solve_cg(rtol=1e-10, fluxes=False)
        assert bits(q) == runs[0][0] and np.all(q.MFL == 0.0) and np.all(q.MFR == 0.0)
    # every row decoupled: x = 0, finite results
    with pkg.Volume(nx, ny, nz) as v:
        v.assemble_from_D(np.zeros((nz, ny, nx)), CL, CR)
        v.init_linear(CL, CR)
        Az, bz = v.get_system()
        assert np.all(vm.decoupled3(Az, bz))
        r = v.solve_cg(rtol=1e-10)
        assert r.converged and r.iters == 0 and r.rel_residual == 0.0 and r.deff_raw == 0.0, r
        assert np.all(v.get_field() == 0.0) and np.all(r.MFL == 0.0) and np.all(r.MFR == 0.0)


def test_refusals_change_nothing(pkg):
    nx, ny, nz = 9, 7, 3
    D, A, b = case(nx, ny, nz)
    L = pkg._capi.load()
    h = C.c_void_p()
    for shape in ((1, 4, 2), (4, 1, 2), (4, 4, 0), (4, 4, -1)):
        assert L.deff_volume_create(0, *shape, C.byref(h)) == EINVAL and not h.value, shape
        with pytest.raises(pkg.DeffError) as ei:
            pkg.Volume(*shape)
        assert ei.value.code == EINVAL
    assert L.deff_volume_create(0, nx, ny, nz, None) == EINVAL
    res = pkg._capi.CGResultC()
    n = nx * ny * nz
    with pkg.Volume(nx, ny, nz) as v:
        hv = v._vol
        # before an assembly, before a field
        assert L.deff_volume_solve_cg(hv, 1e-10, 10, 1, C.byref(res), None, None) == ESTATE
        assert L.deff_volume_get_system(hv, np.zeros(n * 7), np.zeros(n)) == ESTATE
        v.assemble_from_D(D, CL, CR)
        with pytest.raises(pkg.DeffError) as ei:
            v.solve_cg()
        assert ei.value.code == ESTATE and "field" in last_error(pkg)
    with pkg.Volume(nx, ny, nz) as v:
        hv = v._vol
        v.init_linear(CL, CR)
        with pytest.raises(pkg.DeffError) as ei:
            v.solve_cg()
        assert ei.value.code == ESTATE and "system" in last_error(pkg)
        v.assemble_from_D(D, CL, CR)
        x0 = v.get_field()
        sys0 = v.get_system()
        unchanged = lambda: vm.same_bits(v.get_field(), x0) and all(vm.same_bits(a, c) for a, c in zip(v.get_system(), sys0))
        # NULL arguments and bad numbers
        assert L.deff_volume_solve_cg(None, 1e-10, 10, 1, C.byref(res), None, None) == EINVAL
        assert L.deff_volume_solve_cg(hv, 1e-10, 10, 1, None, None, None) == EINVAL
        raw = C.CDLL(pkg.LIB_PATH)                                    # no argtypes: NULL where the binding wants an array
        assert raw.deff_volume_assemble_from_D(hv, None, C.c_double(CL), C.c_double(CR)) == EINVAL
        assert raw.deff_volume_set_field(hv, None) == EINVAL and raw.deff_volume_get_field(hv, None) == EINVAL
        assert raw.deff_volume_get_system(hv, None, None) == EINVAL
        assert L.deff_volume_flux(hv, None, None, None) == EINVAL
        for rtol, max_iter, ce in ((-1.0, 10, 1), (float("nan"), 10, 1), (float("inf"), 10, 1), (1e-10, -1, 1), (1e-10, 10, 0)):
            assert L.deff_volume_solve_cg(hv, rtol, max_iter, ce, C.byref(res), None, None) == EINVAL, (rtol, max_iter, ce)
        with pytest.raises(pkg.DeffError) as ei:
            v.plan_value("tb_T")
        assert ei.value.code == EINVAL
        assert unchanged()
        assert v.plan_value("cg_impl") == 0
        # a negative D cell: its faces' means are negative, the row's a0 with them -- refused by the admissibility pass
        Dn = np.ones((nz, ny, nx))
        Dn[1, 3, 4] = -0.25
        v.assemble_from_D(Dn, CL, CR)
        An, bn = v.get_system()
        assert An[(1 * ny + 3) * nx + 4, 0] < 0.0
        with pytest.raises(pkg.DeffError) as ei:
            v.solve_cg()
        assert ei.value.code == EINVAL and "admissible" in last_error(pkg)
        assert vm.same_bits(v.get_field(), x0)
        assert all(vm.same_bits(a, c) for a, c in zip(v.get_system(), (An, bn)))
        # the same volume with the consistent system goes through
        v.assemble_from_D(D, CL, CR)
        assert unchanged()
        assert v.solve_cg(rtol=1e-10).converged and v.plan_value("cg_impl") == 5


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Nothing else moves

def test_a_volume_leaves_a_2d_solver_alone(pkg):
    nx, ny = 130, 33
    D2 = case(nx, ny, 1)[0][0]

    def run_2d():
        with pkg.Solver(nx, ny) as s:
            s.set_tuning("cg_planes", 1)
            s.assemble_from_D(D2, CL, CR)
            s.init_linear(CL, CR)
            r = s.solve_cg(rtol=1e-10)
            return bits(r), s.get_field(), s.get_system(), s.plan_value("cg_impl"), r.MFL.copy(), r.MFR.copy()

    before = run_2d()
    with pkg.Solver(nx, ny) as s:                                     # a 2-D context alive across the volume's life
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D2, CL, CR)
        s.init_linear(CL, CR)
        with assembled(pkg, 16, 3, 5) as v:
            assert v.solve_cg(rtol=1e-10).converged
        r = s.solve_cg(rtol=1e-10)
        inside = (bits(r), s.get_field(), s.get_system(), s.plan_value("cg_impl"), r.MFL.copy(), r.MFR.copy())
    after = run_2d()
    for got in (inside, after):
        assert got[0] == before[0] and got[3] == before[3]
        assert vm.same_bits(got[1], before[1]) and np.array_equal(got[4], before[4]) and np.array_equal(got[5], before[5])
        assert vm.same_bits(got[2][0], before[2][0]) and vm.same_bits(got[2][1], before[2][1])
