"""The second-order field adjoint on the GPU (deff_adjoint_tangent_rhs_D, deff_solve_adjoint_tangent, deff_field_vjp_hvp_D and
the adjoint tangent's buffer; csrc/kernels_facepass.hpp with FieldHvpPass): the pass bit for bit against the numpy model of the
normative expressions at every strip / seam / pad shape on arbitrary planes, the new right-hand side bit for bit against the
tangent's model on lambda, the whole product against the model on direct solves, the identities that need no reference on the
device (S_w D = -g, symmetry), what the calls leave alone, refusals, and the second derivative of the torch op."""
import ctypes as C
import functools

import numpy as np
import pytest

from field_hvp_model import field_hvp as model
from field_vjp_model import field_vjp as vjp_model
from tangent_model import tangent_rhs
from test_cg_host import block_thomas, decoupled_of, pcg_numpy, rel_l2
from test_gpu_sens_hvp import WALLS
from test_gpu_sensitivity import _refused, device_rows, make_case

pytestmark = pytest.mark.gpu
CURV_MASS_BAR = 1e-12                                    # curv against the model's long-double sum, relative to sum |d hv| (check_map)


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_planes(D, seed):
    """A random direction, non-zero on every cell -- the cells with D == 0 included, where the pass has to ignore it --, and
    random planes for lambda, dx and dlambda (the pass is a function of any six planes)."""
    rng = np.random.default_rng(seed + 311)
    dD = rng.standard_normal(D.shape)
    dD[dD == 0.0] = 1.0
    return dD, rng.standard_normal(D.shape), rng.standard_normal(D.shape), rng.standard_normal(D.shape)


# ---- the pass, bit for bit ----------------------------------------------------------------------------------------------

def check_map(pkg, nx, ny, nimg, CL, CR, kt=0, seed=0):
    """The map equals the model's (array_equal); curv is within 1e-12 of sum |d hv| of the model's long-double sum (the sum has
    no sign, so not relative to itself; the summation order's worst case is about 1 044 x 2^-53 = 1.2e-13 of sum |t|: up to 1 024
    serial additions per lane at kt 64, then the fixed trees) and the same bits on a second call; the four planes are unchanged;
    the device map is the host map with a pad column of 0.  Returns (fhvp_kt, fhvp_items) as used."""
    x, D = make_case(nx, ny, nimg, CL, CR, seed)
    dD, lam, y, m = make_planes(D, seed)
    out = [model(x[k], lam[k], y[k], m[k], D[k], dD[k], CL, CR) for k in range(nimg)]
    want, cv_want = np.stack([h for h, _ in out]), [c for _, c in out]
    rows = nimg * ny
    r2 = lambda a: a.reshape(rows, nx)                   # noqa: E731
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(r2(D), CL, CR)
        s.set_field(r2(x))
        s.set_adjoint(r2(lam))
        s.set_tangent(r2(y))
        s.set_adjoint_tangent(r2(m))
        if kt:
            s.set_tuning("fhvp_kt", kt)
        hv, cv = s.field_vjp_hvp(r2(D), r2(dD), CL, CR)
        hv2, cv2 = s.field_vjp_hvp(r2(D), r2(dD), CL, CR)
        plan = s.plan_value("fhvp_kt"), s.plan_value("fhvp_items")
        assert np.array_equal(s.get_field(), r2(x)) and np.array_equal(s.get_adjoint(), r2(lam))
        assert np.array_equal(s.get_tangent(), r2(y)) and np.array_equal(s.get_adjoint_tangent(), r2(m))
        p, pitch = s.device_field_vjp_hvp_ptr()
        dev = device_rows(p, rows, pitch)
        assert pitch == s.device_field_ptr()[1] == 8 * (nx + (nx & 1))
        assert np.array_equal(dev[:, :nx], hv.reshape(rows, nx)) and np.all(dev[:, nx:] == 0.0)
        pm, pitch_m = s.device_adjoint_tangent_ptr()
        devm = device_rows(pm, rows, pitch_m)
        assert pitch_m == pitch and np.array_equal(devm[:, :nx], r2(m)) and np.all(devm[:, nx:] == 0.0)
    hv, hv2 = hv.reshape(nimg, ny, nx), hv2.reshape(nimg, ny, nx)
    cv, cv2 = np.atleast_1d(cv), np.atleast_1d(cv2)
    d = np.where(D == 0.0, 0.0, dD)
    for k in range(nimg):
        bad = np.argwhere(hv[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), hv[k][tuple(bad[0])], want[k][tuple(bad[0])])
        mass = float(np.sum(np.abs(d[k] * want[k])))
        off = abs(float(np.longdouble(cv[k]) - cv_want[k]))
        print(f"field hvp {nimg} x {nx}x{ny} kt {plan[0]} image {k}: curv {cv[k]:.6e}, off the model's by {off / mass:.3e} of sum |d hv|")
        assert off <= CURV_MASS_BAR * mass, (k, cv[k], cv_want[k], mass)
    assert np.array_equal(hv, hv2) and np.array_equal(cv, cv2)
    assert np.all(hv[D == 0.0] == 0.0) and np.any(hv != 0.0) and np.all(np.isfinite(hv))
    return plan


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 5), (127, 17), (129, 17), (130, 64), (130, 71), (258, 9), (1030, 37)])
def test_map_matches_model(pkg, nx, ny, CL, CR):
    kt, items = check_map(pkg, nx, ny, 1, CL, CR, seed=nx * 100 + ny)
    assert kt == 1 and items == ((nx + 127) // 128) * ((ny + 7) // 8)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nimg,nx,ny", [(3, 33, 20), (5, 130, 69)])
def test_map_matches_model_stacks(pkg, nimg, nx, ny, CL, CR):
    """Every image of a stack has its own first and last row."""
    check_map(pkg, nx, ny, nimg, CL, CR, seed=nimg)


@pytest.mark.parametrize("nimg,nx,ny", [(1, 130, 71), (5, 130, 69)])
@pytest.mark.parametrize("kt", [1, 2, 64])
def test_map_matches_model_at_work_item_seams(pkg, nimg, nx, ny, kt):
    """"fhvp_kt": 9 tile rows, 2 strips -- kt = 1 has a seam every 8 rows (9 items per strip), kt = 2 every 16 (5 items, the last
    one 7 rows short), kt = 64 is clipped to the image (one item per strip, no seam)."""
    used, items = check_map(pkg, nx, ny, nimg, 0.0, 1.0, kt=kt, seed=7 + kt)
    assert (used, items) == {1: (1, 18), 2: (2, 10), 64: (9, 2)}[kt]


def test_map_matches_model_large(pkg):
    """2050 x 1537: 17 strips (the last one 2 columns wide), 193 tile rows, an odd height."""
    kt, items = check_map(pkg, 2050, 1537, 1, 0.0, 1.0, seed=99)
    assert items == 17 * ((193 + kt - 1) // kt)


# ---- the new right-hand side ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nimg,nx,ny", [(1, 129, 17), (5, 130, 69)])
def test_adjoint_tangent_rhs_matches_model(pkg, nimg, nx, ny):
    """q is the tangent's model on lambda with both wall values 0, bit for bit; norm2 within 1e-13 relative of the long-double
    sum; and the tangent's own map and dx are bitwise what they were."""
    CL, CR = 2.0, -1.0
    x, D = make_case(nx, ny, nimg, CL, CR, 40 + nimg)
    dD, lam, y, _ = make_planes(D, 40 + nimg)
    rows = nimg * ny
    r2 = lambda a: a.reshape(rows, nx)                   # noqa: E731
    out = [tangent_rhs(lam[k], D[k], dD[k], 0.0, 0.0) for k in range(nimg)]
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(r2(D), CL, CR)
        s.set_field(r2(x))
        s.set_adjoint(r2(lam))
        s.set_tangent(r2(y))
        r0, _ = s.tangent_rhs(r2(D), r2(dD), CL, CR)
        pr, pitch = s.device_tangent_rhs_ptr()
        dev_r = device_rows(pr, rows, pitch)
        plan_tan = s.plan_value("tan_kt"), s.plan_value("tan_items")
        q, n2 = s.adjoint_tangent_rhs(r2(D), r2(dD))
        q2, n22 = s.adjoint_tangent_rhs(r2(D), r2(dD))
        assert s.device_tangent_rhs_ptr() == (pr, pitch) and np.array_equal(device_rows(pr, rows, pitch), dev_r)
        assert (s.plan_value("tan_kt"), s.plan_value("tan_items")) == plan_tan
        assert np.array_equal(s.get_tangent(), r2(y)) and np.array_equal(s.get_adjoint(), r2(lam))
        assert np.array_equal(s.get_field(), r2(x))
    q, n2 = q.reshape(nimg, ny, nx), np.atleast_1d(n2)
    assert np.array_equal(q, q2.reshape(nimg, ny, nx)) and np.array_equal(n2, np.atleast_1d(n22))
    assert not np.array_equal(q, np.asarray(r0).reshape(nimg, ny, nx))
    for k in range(nimg):
        assert np.array_equal(q[k], out[k][0]), k
        rel = abs(float(np.longdouble(n2[k]) - out[k][1])) / float(out[k][1])
        print(f"adjoint tangent rhs {nimg} x {nx}x{ny} image {k}: norm2 {n2[k]:.6e}, off the model's by {rel:.3e}")
        assert rel <= 1e-13, (k, n2[k], out[k][1])


# ---- the whole product against the direct solves, and the identities ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def direct_case(nx, ny):
    """One system per shape, shared and left unchanged: D = exp(2 N(0, 1)) with zero cells, two directions v and u, a gradient
    w; the model on the direct solves (decoupled cells fixed at 0) for v; and what the model makes of numpy's float64 CG fields
    stopped at rtol 1e-13: its distance from that, its |S_w D + g| / |g| and its miss of <u, S_w v> = <v, S_w u>.  The
    reference's own error, which sets the bars."""
    import oracle_binding as ob
    ob.build()
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + ny + 2)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    D[rng.random((ny, nx)) < 0.03] = 0.0
    D[ny // 2, nx // 2 - 1:nx // 2 + 1] = 0.0
    D[3, 0] = 0.0
    v = D * rng.standard_normal((ny, nx)) + np.where(D == 0.0, 1.0, 0.0)
    u = D * rng.standard_normal((ny, nx)) + np.where(D == 0.0, -1.0, 0.0)
    w = rng.standard_normal((ny, nx))
    A, b = ob.discretize(D, CL, CR)
    dec = decoupled_of(A, b).reshape(ny, nx)
    zero = np.zeros((ny, nx))

    def product(solve, x, lam, d):
        r = np.where(dec, 0.0, tangent_rhs(x, D, d, CL, CR)[0])
        q = np.where(dec, 0.0, tangent_rhs(lam, D, d, 0.0, 0.0)[0])
        return model(x, lam, solve(r), solve(q), D, d, CL, CR)

    direct = lambda rhs: block_thomas(A, rhs.ravel(), nx, ny, fixed=dec.ravel())      # noqa: E731
    cg = lambda rhs: pcg_numpy(A, rhs.ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-13).x.reshape(ny, nx)   # noqa: E731
    wm = np.where(dec, 0.0, w)
    xd = block_thomas(A, b, nx, ny, fixed=dec.ravel())
    hv_d, curv_d = product(direct, xd, direct(wm), v)
    # the same on numpy's CG fields
    tx = pcg_numpy(A, b, ob.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-13).x.reshape(ny, nx)
    tl = cg(wm)
    hv_np, hu_np, hD_np = (product(cg, tx, tl, d)[0] for d in (v, u, D))
    g_np = vjp_model(tx, tl, D, CL, CR)[0]
    dv, du = np.where(D == 0.0, 0.0, v), np.where(D == 0.0, 0.0, u)
    lhs = float(np.sum(du * hv_np))
    out = dict(CL=CL, CR=CR, D=D, v=v, u=u, w=w, dv=dv, du=du, hv_d=hv_d, curv_d=float(curv_d), d_ref=rel_l2(hv_np, hv_d),
               euler_np=float(np.max(np.abs(hD_np + g_np)) / np.max(np.abs(g_np))),
               sym_np=abs(lhs - float(np.sum(dv * hu_np))) / abs(lhs))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_field_hvp_end_to_end(pkg, nx, ny):
    """solve_cg(1e-13), solve_adjoint(w, 1e-13), then field_hvp(rtol 1e-13) along v, u and D.  S_w v against the model on the
    direct solves: bar max(1e-10, 10 d_ref), d_ref the same distance when the model is fed numpy's float64 CG fields at that
    rtol.  |S_w D + g| / |g| and the miss of <u, S_w v> = <v, S_w u>: within 10 x the same figures from numpy's CG fields, with
    the floors 1e-9 and 1e-12."""
    c = direct_case(nx, ny)
    CL, CR, D = c["CL"], c["CR"], c["D"]
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        rx = s.solve_cg(rtol=1e-13)
        x = s.get_field()
        rl = s.solve_adjoint(c["w"], rtol=1e-13)
        lam = s.get_adjoint()
        g, _ = s.field_vjp(D, CL, CR)
        hv, cv = s.field_hvp(D, c["v"], CL, CR, rtol=1e-13)
        hu, cu = s.field_hvp(D, c["u"], CL, CR, rtol=1e-13)
        hD, cD = s.field_hvp(D, D, CL, CR, rtol=1e-13)
        assert np.array_equal(s.get_field(), x) and np.array_equal(s.get_adjoint(), lam)
    assert rx.converged and rl.converged
    d = rel_l2(hv, c["hv_d"])
    euler = float(np.max(np.abs(hD + g)) / np.max(np.abs(g)))
    lhs, rhs = float(np.sum(c["du"] * hv)), float(np.sum(c["dv"] * hu))
    sym = abs(lhs - rhs) / abs(lhs)
    print(f"field hvp end to end {nx}x{ny}: d {d:.3e} (numpy CG {c['d_ref']:.3e}); |S D + g| / |g| {euler:.3e} (numpy CG "
          f"{c['euler_np']:.3e}); <u, S v> {lhs:.9e} <v, S u> {rhs:.9e} rel {sym:.3e} (numpy CG {c['sym_np']:.3e}); curv {cv:.6e} "
          f"{cu:.6e} (direct {c['curv_d']:.6e})")
    assert d <= max(1e-10, 10 * c["d_ref"]), (d, c["d_ref"])
    assert euler <= max(1e-9, 10 * c["euler_np"]), (euler, c["euler_np"])
    assert sym <= max(1e-12, 10 * c["sym_np"]), (sym, c["sym_np"])
    assert np.all(hv[D == 0.0] == 0.0)


# ---- what the calls leave alone, refusals ------------------------------------------------------------------------------------

def test_calls_leave_everything_else_alone(pkg):
    """After field_vjp_hvp: field, system, lambda, dx, dlambda and the rhs, vjp, sensitivity and Deff-hvp maps are bitwise what
    they were; after solve_adjoint_tangent: all of these except dlambda."""
    nx, ny, nimg = 33, 20, 2                             # odd width: the device maps have a pad column
    CL, CR = 2.0, -1.0
    x, D = make_case(nx, ny, nimg, CL, CR, 21)
    dD, lam, y, m = make_planes(D, 21)
    rows = nimg * ny
    x2, D2, dD2, lam2, y2, m2 = (a.reshape(rows, nx) for a in (x, D, dD, lam, y, m))
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(D2, CL, CR)
        s.set_field(x2)
        A0, b0 = s.get_system()
        s.set_adjoint(lam2)
        s.set_tangent(y2)
        s.set_adjoint_tangent(m2)
        s.tangent_rhs(D2, dD2, CL, CR)
        s.adjoint_tangent_rhs(D2, dD2)
        s.set_adjoint_tangent(m2)                        # (a new right-hand side made dlambda invalid)
        s.field_vjp(D2, CL, CR)
        s.sensitivity(D2, CL, CR)
        s.sens_hvp(D2, dD2, CL, CR)
        getters = (s.device_tangent_rhs_ptr, s.device_field_vjp_ptr, s.device_sensitivity_ptr, s.device_sens_hvp_ptr)
        ptrs = [f() for f in getters]
        maps = [device_rows(p, rows, pitch) for p, pitch in ptrs]

        def unchanged(dl):
            assert [f() for f in getters] == ptrs
            for (p, pitch), a in zip(ptrs, maps):
                assert np.array_equal(device_rows(p, rows, pitch), a)
            assert np.array_equal(s.get_field(), x2) and np.array_equal(s.get_adjoint(), lam2)
            assert np.array_equal(s.get_tangent(), y2)
            if dl is not None:
                assert np.array_equal(s.get_adjoint_tangent(), dl)
            A1, b1 = s.get_system()
            assert np.array_equal(A1, A0) and np.array_equal(b1, b0)

        hv, _ = s.field_vjp_hvp(D2, dD2, CL, CR)
        assert np.any(hv != 0.0)
        unchanged(m2)
        ph = s.device_field_vjp_hvp_ptr()
        devh = device_rows(ph[0], rows, ph[1])
        s.adjoint_tangent_rhs(D2, dD2)
        assert all(r.converged for r in s.solve_adjoint_tangent(rtol=1e-10))
        unchanged(None)
        assert s.device_field_vjp_hvp_ptr() == ph and np.array_equal(device_rows(ph[0], rows, ph[1]), devh)
        # the dlambda a solve left serves as well as a caller's own, and the pass leaves it alone too
        dl = s.get_adjoint_tangent()
        assert not np.array_equal(dl, m2)
        h1, c1 = s.field_vjp_hvp(D2, dD2, CL, CR)
        unchanged(dl)
        s.set_adjoint_tangent(dl)
        h2, c2 = s.field_vjp_hvp(D2, dD2, CL, CR)
        assert np.array_equal(h1, h2) and np.array_equal(c1, c2)


def test_refusals_leave_the_map_alone(pkg, oracle):
    nx, ny = 33, 20                                      # odd width: the device map has a pad column
    CL, CR = 0.0, 1.0
    x, D = make_case(nx, ny, 1, CL, CR, 3)
    x, D = x[0], D[0]
    dD, lam, y, m = make_planes(D, 3)
    L = pkg._capi.load()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)      # noqa: E731
    res = (pkg._capi.CGResultC * 1)()
    with pkg.Solver(nx, ny) as s:
        hvp = lambda: s.field_vjp_hvp(D, dD, CL, CR)     # noqa: E731
        _refused(pkg, s.device_field_vjp_hvp_ptr, -5)    # DEFF_ESTATE: no map yet
        _refused(pkg, lambda: s.set_adjoint_tangent(m), -5, "no system")
        _refused(pkg, hvp, -5, "no field")
        s.set_field(x)
        _refused(pkg, hvp, -5, "adjoint field")
        _refused(pkg, lambda: s.adjoint_tangent_rhs(D, dD), -5, "adjoint field")
        s.assemble_from_D(D, CL, CR)
        s.set_field(x)
        _refused(pkg, hvp, -5, "adjoint field")
        _refused(pkg, s.solve_adjoint_tangent, -5, "right-hand side")
        s.set_adjoint(lam)
        _refused(pkg, hvp, -5, "no tangent field")
        s.set_tangent(y)
        _refused(pkg, hvp, -5, "adjoint tangent")        # before any solve or set_adjoint_tangent
        _refused(pkg, s.get_adjoint_tangent, -5, "adjoint tangent")
        _refused(pkg, s.device_adjoint_tangent_ptr, -5, "adjoint tangent")
        _refused(pkg, s.solve_adjoint_tangent, -5, "right-hand side")
        s.adjoint_tangent_rhs(D, dD)
        _refused(pkg, hvp, -5, "adjoint tangent")        # a right-hand side is no dlambda
        _refused(pkg, s.device_field_vjp_hvp_ptr, -5)
        s.set_adjoint_tangent(m)
        hv0, cv0 = hvp()
        p, pitch = s.device_field_vjp_hvp_ptr()
        dev = device_rows(p, ny, pitch)
        assert np.array_equal(dev[:, :nx], hv0) and np.all(dev[:, nx:] == 0.0)

        def unchanged():
            assert s.device_field_vjp_hvp_ptr() == (p, pitch) and np.array_equal(device_rows(p, ny, pitch), dev)

        # NULL arguments
        assert L.deff_field_vjp_hvp_D(s._ctx, None, vp(dD), CL, CR, None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        assert L.deff_field_vjp_hvp_D(s._ctx, vp(D), None, CL, CR, None, None, None) == -1 and b"dD is NULL" in L.deff_last_error()
        assert L.deff_adjoint_tangent_rhs_D(s._ctx, None, vp(dD), None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        assert L.deff_adjoint_tangent_rhs_D(s._ctx, vp(D), None, None, None, None) == -1 and b"dD is NULL" in L.deff_last_error()
        assert L.deff_device_field_vjp_hvp(s._ctx, None, None) == -1
        assert L.deff_set_adjoint_tangent(s._ctx, None) == -1
        assert L.deff_get_adjoint_tangent(s._ctx, None) == -1
        assert L.deff_solve_adjoint_tangent(s._ctx, 1e-10, 100, 1, None) == -1
        unchanged()
        assert np.array_equal(s.get_adjoint_tangent(), m)
        # CR == CL is allowed: nothing is divided by it; hv and curv may each be NULL
        assert np.all(np.isfinite(s.field_vjp_hvp(D, dD, 1.0, 1.0)[0]))
        assert np.array_equal(hvp()[0], hv0)
        assert L.deff_field_vjp_hvp_D(s._ctx, vp(D), vp(dD), CL, CR, None, None, None) == 0
        unchanged()
        # a new lambda makes dlambda and the right-hand side stale
        for again in (lambda: s.set_adjoint(lam), lambda: s.solve_adjoint(lam, rtol=1e-6)):
            s.adjoint_tangent_rhs(D, dD)
            s.set_adjoint_tangent(m)
            assert np.array_equal(hvp()[0], hv0)
            again()
            s.set_adjoint(lam)
            _refused(pkg, hvp, -5, "adjoint tangent")
            _refused(pkg, s.get_adjoint_tangent, -5)
            assert L.deff_solve_adjoint_tangent(s._ctx, 1e-10, 100, 1, res) == -5 and b"right-hand side" in L.deff_last_error()
            unchanged()
        # every call that replaces the system or the image invalidates dlambda: the pass refuses, the old map stays
        A, b = s.get_system()
        for again in (lambda: s.assemble_2phase(1e-3, 1.0, CL, CR), lambda: s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR),
                      lambda: s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR), lambda: s.assemble_from_D(D, CL, CR),
                      lambda: s.set_system(A, b, D, CL, CR), lambda: s.synth_image(1, 0),
                      lambda: s.set_image(oracle.synth_mask(nx, ny, 12345, 0))):
            s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
            s.assemble_from_D(D, CL, CR)
            s.set_field(x)
            s.set_adjoint(lam)
            s.set_tangent(y)
            s.adjoint_tangent_rhs(D, dD)
            s.set_adjoint_tangent(m)
            assert np.array_equal(hvp()[0], hv0)
            again()
            s.set_field(x)
            s.set_adjoint(lam)
            _refused(pkg, hvp, -5, "no tangent field")
            try:
                s.set_tangent(y)
                _refused(pkg, hvp, -5, "adjoint tangent")
            except pkg.DeffError as e:                   # a new image has no system yet
                assert e.code == -5 and "no system" in str(e)
            _refused(pkg, s.get_adjoint_tangent, -5, "adjoint tangent")
            unchanged()
    with pkg.SlabRank(nx + 1, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(oracle.synth_mask(nx + 1, ny, 12345, 0))
        sr.assemble_2phase(1e-3, 1.0, CL, CR)
        sr.init_linear(CL, CR)
        x0 = sr.get_field()
        out = np.zeros((ny, nx + 1))
        one = np.ones((ny, nx + 1))
        assert L.deff_field_vjp_hvp_D(sr._ctx, vp(one), vp(one), CL, CR, vp(out), None, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert L.deff_adjoint_tangent_rhs_D(sr._ctx, vp(one), vp(one), vp(out), None, None) == -1 and b"row-slab" in L.deff_last_error()
        assert L.deff_set_adjoint_tangent(sr._ctx, vp(one)) == -1 and b"row-slab" in L.deff_last_error()
        assert L.deff_solve_adjoint_tangent(sr._ctx, 1e-10, 100, 1, res) == -1 and b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0) and np.all(out == 0.0)


# ---- torch ---------------------------------------------------------------------------------------------------------------

def test_torch_second_order(pkg):
    """concentration_field twice differentiated under L = 1/2 |x - x_obs|^2, at 12 x 9 on cpu and cuda and on a stack of 2 on a
    passed solver: grad(create_graph=True) then (g * v).sum().backward() equals the hand composition on a Solver -- field_vjp
    after solve_adjoint(J v), plus field_hvp with w = x - x_obs -- (array_equal); torch.autograd.functional.hvp is within 1e-10
    (the end-to-end rule's floor) of it; it matches central differences of the first-order D.grad along v (bar: 10 x the gap
    between the steps 1e-5 and 1e-6, the gap below 1e-4); a linear loss w^T x gives S_w v alone; and first-order backward is
    bitwise the library calls made by hand and builds no graph."""
    import torch
    from effectivediffusivityfvm_amd import concentration_field
    nx, ny = 12, 9
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(17)
    Dn = np.exp(2.0 * rng.standard_normal((2, ny, nx)))
    vn = Dn * rng.standard_normal((2, ny, nx))
    xo = rng.random((2, ny, nx))
    wl = rng.standard_normal((2, ny, nx))                # the linear loss's gradient

    def by_hand(s, D, v, x_obs, w_lin):
        """(g, S_w v + J^T J v) of the quadratic loss, and S_w v of the linear one."""
        nimg = D.shape[0] if D.ndim == 3 else 1
        D2, v2 = D.reshape(nimg * ny, nx), v.reshape(nimg * ny, nx)
        ok = lambda rs: all(r.converged for r in (rs if isinstance(rs, list) else [rs]))      # noqa: E731
        s.assemble_from_D(D2, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        assert ok(s.solve_cg(rtol=1e-12, fluxes=False))
        x = s.get_field()
        w = x - x_obs.reshape(nimg * ny, nx)
        s.assemble_from_D(D2, CL, CR)
        s.set_field(x)
        assert ok(s.solve_adjoint(w, rtol=1e-12))
        g, _ = s.field_vjp(D2, CL, CR)
        hv, _ = s.field_hvp(D2, v2, CL, CR, rtol=1e-12)
        Jv = s.get_tangent()
        assert ok(s.solve_adjoint(Jv, rtol=1e-12))
        gn, _ = s.field_vjp(D2, CL, CR)
        assert ok(s.solve_adjoint(w_lin.reshape(nimg * ny, nx), rtol=1e-12))
        hl, _ = s.field_hvp(D2, v2, CL, CR, rtol=1e-12)
        return tuple(np.asarray(a).reshape(D.shape) for a in (g, np.asarray(hv) + np.asarray(gn), hl))

    def loss(q, x_obs, solver=None):
        return 0.5 * ((concentration_field(q, CL, CR, solver=solver) - x_obs) ** 2).sum()

    with pkg.Solver(nx, ny) as s:
        g_hand, hv_hand, hl_hand = by_hand(s, Dn[0], vn[0], xo[0], wl[0])
    assert np.any(hv_hand != 0.0) and np.any(hl_hand != 0.0)

    def grad_at(Dq, dev):
        Dt = torch.tensor(Dq, dtype=torch.float64, device=dev, requires_grad=True)
        loss(Dt, torch.tensor(xo[0], dtype=torch.float64, device=dev)).backward()
        return Dt.grad.cpu().numpy()

    for dev in ("cpu", "cuda"):
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)      # noqa: E731
        D = t(Dn[0]).requires_grad_()
        v, x_obs = t(vn[0]), t(xo[0])
        (g,) = torch.autograd.grad(loss(D, x_obs), D, create_graph=True)
        assert g.requires_grad and np.array_equal(g.detach().cpu().numpy(), g_hand)
        (g * v).sum().backward()
        assert D.grad.shape == D.shape and D.grad.device == D.device and D.grad.dtype == torch.float64
        hv = D.grad.cpu().numpy()
        assert np.array_equal(hv, hv_hand)
        _, hv_f = torch.autograd.functional.hvp(lambda q: loss(q, x_obs), D.detach(), v)
        d_f = rel_l2(hv_f.cpu().numpy(), hv_hand)
        print(f"concentration_field functional.hvp on {dev}: off the hand composition by {d_f:.3e}")
        assert d_f <= 1e-10, d_f
        # a linear loss: S_w v alone
        D2 = t(Dn[0]).requires_grad_()
        (gl,) = torch.autograd.grad((concentration_field(D2, CL, CR) * t(wl[0])).sum(), D2, create_graph=True)
        (gl * v).sum().backward()
        assert np.array_equal(D2.grad.cpu().numpy(), hl_hand)
        # first order: what it was, bitwise, and no graph without create_graph
        assert np.array_equal(grad_at(Dn[0], dev), g_hand)
        D1 = t(Dn[0]).requires_grad_()
        (g1,) = torch.autograd.grad(loss(D1, x_obs), D1)
        assert not g1.requires_grad and g1.grad_fn is None and np.array_equal(g1.cpu().numpy(), g_hand)
        fd5 = (grad_at(Dn[0] + 1e-5 * vn[0], dev) - grad_at(Dn[0] - 1e-5 * vn[0], dev)) / 2e-5
        fd6 = (grad_at(Dn[0] + 1e-6 * vn[0], dev) - grad_at(Dn[0] - 1e-6 * vn[0], dev)) / 2e-6
        scale = np.max(np.abs(hv))
        gap, err = np.max(np.abs(fd5 - fd6)) / scale, np.max(np.abs(hv - fd5)) / scale
        print(f"concentration_field second order on {dev}: gap {gap:.3e} err {err:.3e}")
        assert gap < 1e-4, gap
        assert err <= 10.0 * gap, (err, gap)
    # a stack of 2 on a solver that is passed in and stays open
    with pkg.Solver(nx, ny, nimg=2) as s:
        g_hand2, hv_hand2, _ = by_hand(s, Dn, vn, xo, wl)
        t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")   # noqa: E731
        D = t(Dn).requires_grad_()
        v, x_obs = t(vn), t(xo)
        (g,) = torch.autograd.grad(loss(D, x_obs, s), D, create_graph=True)
        s.init_linear(CL, CR)                            # whatever happens to the passed solver in between
        (g * v).sum().backward()
        s.init_linear(CL, CR)                            # the passed solver is still open
        _, hv_f = torch.autograd.functional.hvp(lambda q: loss(q, x_obs, s), D.detach(), v)
    assert np.array_equal(g.detach().cpu().numpy(), g_hand2)
    assert np.array_equal(D.grad.cpu().numpy(), hv_hand2)
    assert rel_l2(hv_f.cpu().numpy(), hv_hand2) <= 1e-10
