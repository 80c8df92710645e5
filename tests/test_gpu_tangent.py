"""The field tangent on the GPU (deff_tangent_rhs_D, deff_solve_tangent; csrc/kernels_facepass.hpp with TanPass): the pass bit
for bit against the numpy model of the normative expressions at every strip / seam / pad shape, the solve bit for bit against
deff_solve_adjoint given the same right-hand side from the host, against the direct solve, the dot-product identity with the
field adjoint on converged fields, what the calls leave alone, refusals and the torch ops' jvp."""
import ctypes as C
import functools

import numpy as np
import pytest

from field_vjp_model import field_vjp as vjp_model
from tangent_model import tangent_rhs as model
from test_cg_host import block_thomas, decoupled_of, pcg_numpy, rel_l2
from test_gpu_sensitivity import _refused, device_rows, make_case

pytestmark = pytest.mark.gpu

WALLS = [(0.0, 1.0), (2.0, -1.0)]
NORM2_BAR = 1e-13                                        # norm2 against the model's long-double sum, relative to it


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_direction(D, seed):
    """A random direction, non-zero on every cell -- the cells with D == 0 included, where the pass has to ignore it."""
    rng = np.random.default_rng(seed + 177)
    dD = rng.standard_normal(D.shape)
    dD[dD == 0.0] = 1.0
    return dD


# ---- the pass, bit for bit ----------------------------------------------------------------------------------------------

def check_map(pkg, nx, ny, nimg, CL, CR, kt=0, seed=0):
    """The map equals the model's (array_equal), norm2 is within 1e-13 sum r^2 of the model's long-double sum and the same
    bits on a second call; the field is unchanged.  Returns (tan_kt, tan_items) as used."""
    x, D = make_case(nx, ny, nimg, CL, CR, seed)
    dD = make_direction(D, seed)
    out = [model(x[k], D[k], dD[k], CL, CR) for k in range(nimg)]
    want, n2_want = np.stack([r for r, _ in out]), [n for _, n in out]
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_field(x.reshape(nimg * ny, nx))
        if kt:
            s.set_tuning("tan_kt", kt)
        r, n2 = s.tangent_rhs(D.reshape(nimg * ny, nx), dD.reshape(nimg * ny, nx), CL, CR)
        r2, n22 = s.tangent_rhs(D.reshape(nimg * ny, nx), dD.reshape(nimg * ny, nx), CL, CR)
        plan = s.plan_value("tan_kt"), s.plan_value("tan_items")
        assert np.array_equal(s.get_field(), x.reshape(nimg * ny, nx))
        p, pitch = s.device_tangent_rhs_ptr()
        dev = device_rows(p, nimg * ny, pitch)
        assert pitch == s.device_field_ptr()[1] == 8 * (nx + (nx & 1))
        assert np.array_equal(dev[:, :nx], r.reshape(nimg * ny, nx)) and np.all(dev[:, nx:] == 0.0)
    r, r2 = r.reshape(nimg, ny, nx), r2.reshape(nimg, ny, nx)
    n2, n22 = np.atleast_1d(n2), np.atleast_1d(n22)
    for k in range(nimg):
        bad = np.argwhere(r[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), r[k][tuple(bad[0])], want[k][tuple(bad[0])])
        size = float(n2_want[k])
        rel = abs(float(np.longdouble(n2[k]) - n2_want[k])) / size
        print(f"tangent rhs {nimg} x {nx}x{ny} kt {plan[0]} image {k}: norm2 {n2[k]:.6e}, off the model's by {rel:.3e} of it")
        assert rel <= NORM2_BAR, (k, n2[k], n2_want[k])
    assert np.array_equal(r, r2) and np.array_equal(n2, n22)
    assert np.all(r[D == 0.0] == 0.0) and np.any(r != 0.0)
    return plan


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 5), (127, 17), (129, 17), (130, 71), (258, 9), (1030, 37)])
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
    """"tan_kt": 9 tile rows, 2 strips -- kt = 1 has a seam every 8 rows (9 items per strip), kt = 2 every 16 (5 items, the last
    one 7 rows short), kt = 64 is clipped to the image (one item per strip, no seam)."""
    used, items = check_map(pkg, nx, ny, nimg, 0.0, 1.0, kt=kt, seed=7 + kt)
    assert (used, items) == {1: (1, 18), 2: (2, 10), 64: (9, 2)}[kt]


def test_map_matches_model_large(pkg):
    """2050 x 1537: 17 strips (the last one 2 columns wide), 193 tile rows, an odd height."""
    kt, items = check_map(pkg, 2050, 1537, 1, 0.0, 1.0, seed=99)
    assert items == 17 * ((193 + kt - 1) // kt)


# ---- the solve, bit for bit, against the adjoint solve of the same right-hand side --------------------------------------------

@pytest.mark.parametrize("nimg,nx,ny", [(1, 130, 71), (1, 33, 40), (3, 33, 20)])
def test_tangent_solve_equals_adjoint_solve_of_the_map(pkg, nimg, nx, ny):
    """get_tangent() is lambda of solve_adjoint(w = r) on the same context: the same bits, iterations and residual, under
    cg_fold 0 / 1 and check_every 1, 7, 64.  Afterwards lambda, the rhs map, the field, the system and the vjp map are what
    they were."""
    CL, CR = 2.0, -1.0
    x, D = make_case(nx, ny, nimg, CL, CR, nx + ny)
    dD = make_direction(D, nx)
    D2, x2 = D.reshape(nimg * ny, nx), x.reshape(nimg * ny, nx)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(D2, CL, CR)
        s.set_field(x2)
        A0, b0 = s.get_system()
        dec = decoupled_of(A0, b0).reshape(nimg * ny, nx)
        assert dec.any()
        r, _ = s.tangent_rhs(D2, dD.reshape(nimg * ny, nx), CL, CR)
        r = r.reshape(nimg * ny, nx)
        pr, pitch = s.device_tangent_rhs_ptr()
        map0 = device_rows(pr, nimg * ny, pitch)
        for fold, every in ((0, 64), (1, 64), (0, 1), (0, 7), (1, 7)):
            s.set_tuning("cg_fold", fold)
            ra = s.solve_adjoint(r, rtol=1e-11, check_every=every)
            ra = ra if isinstance(ra, list) else [ra]
            lam = s.get_adjoint()
            g0, e0 = s.field_vjp(D2, CL, CR)
            pv, _ = s.device_field_vjp_ptr()
            vjp0 = device_rows(pv, nimg * ny, pitch)
            rt = s.solve_tangent(rtol=1e-11, check_every=every)
            rt = rt if isinstance(rt, list) else [rt]
            dx = s.get_tangent()
            assert s.plan_value("cg_impl") == 3 and s.plan_value("cg_fold") == fold
            bad = np.argwhere(dx != lam)
            assert bad.size == 0, (fold, every, len(bad), bad[:5].tolist())
            assert np.all(dx[dec] == 0.0) and dx.any()
            for k in range(nimg):
                assert (rt[k].iters, rt[k].rel_residual, rt[k].converged) == (ra[k].iters, ra[k].rel_residual, ra[k].converged)
                assert rt[k].converged and rt[k].iters > 10 and rt[k].deff_raw == 0.0 and rt[k].loop_ms > 0.0
            pd, pitch_d = s.device_tangent_ptr()
            dev = device_rows(pd, nimg * ny, pitch_d)
            assert pitch_d == pitch and np.array_equal(dev[:, :nx], dx) and np.all(dev[:, nx:] == 0.0)
            # what the solve leaves alone
            assert np.array_equal(s.get_adjoint(), lam)
            assert s.device_tangent_rhs_ptr() == (pr, pitch) and np.array_equal(device_rows(pr, nimg * ny, pitch), map0)
            assert np.array_equal(s.get_field(), x2)
            A1, b1 = s.get_system()
            assert np.array_equal(A1, A0) and np.array_equal(b1, b0)
            assert s.device_field_vjp_ptr()[0] == pv and np.array_equal(device_rows(pv, nimg * ny, pitch), vjp0)
        print(f"tangent solve {nimg} x {nx}x{ny}: {[q.iters for q in rt]} iterations, rel {[q.rel_residual for q in rt]}")


# ---- against the direct solves, and the dot product ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def direct_case(nx, ny):
    """One system per shape, shared and left unchanged: D = exp(2 N(0, 1)) with zero cells, a direction dD and a weight w; the
    direct solves x = A^-1 b and dx = A^-1 r' (r' the model's map on x, decoupled cells fixed at 0); and what numpy's float64
    CG stopped at rtol 1e-13 leaves: its distance from dx on the same r', and -- with every field its own -- its miss of the
    dot-product identity <w', dx> = <field_vjp(x, lambda, D), d>.  The reference's own error, which sets the bars."""
    import oracle_binding as ob
    ob.build()
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    D[rng.random((ny, nx)) < 0.03] = 0.0
    D[ny // 2, nx // 2 - 1:nx // 2 + 1] = 0.0
    D[3, 0] = 0.0
    dD = D * rng.standard_normal((ny, nx)) + np.where(D == 0.0, 1.0, 0.0)
    w = rng.standard_normal((ny, nx))
    A, b = ob.discretize(D, CL, CR)
    dec = decoupled_of(A, b).reshape(ny, nx)
    xd = block_thomas(A, b, nx, ny, fixed=dec.ravel())
    rp = np.where(dec, 0.0, model(xd, D, dD, CL, CR)[0])
    dxd = block_thomas(A, rp.ravel(), nx, ny, fixed=dec.ravel())
    zero = np.zeros((ny, nx))
    t_dx = pcg_numpy(A, rp.ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-13)
    # the identity on numpy's CG fields
    wp = np.where(dec, 0.0, w)
    d = np.where(D == 0.0, 0.0, dD)
    tx = pcg_numpy(A, b, ob.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-13)
    tr = np.where(dec, 0.0, model(tx.x, D, dD, CL, CR)[0])
    tdx = pcg_numpy(A, tr.ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-13)
    tl = pcg_numpy(A, wp.ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-13)
    g_np, _ = vjp_model(tx.x, tl.x, D, CL, CR)
    lhs = float(np.sum(wp * tdx.x))
    out = dict(CL=CL, CR=CR, D=D, dD=dD, d=d, w=w, wp=wp, dec=dec, xd=xd, dxd=dxd, d_dx=rel_l2(t_dx.x, dxd), it_dx=t_dx.iters,
               dot_np=abs(lhs - float(np.sum(g_np * d))) / abs(lhs))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_tangent_against_direct_solve(pkg, nx, ny):
    """dx at rtol 1e-13 against block_thomas(A, r', fixed = decoupled), the field being the direct solve's.  Bar as for
    lambda in test_gpu_field_vjp.py: max(1e-10, 10 d_ref), d_ref the same distance for numpy's float64 CG at the same rtol."""
    c = direct_case(nx, ny)
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(c["D"], c["CL"], c["CR"])
        s.set_field(c["xd"])
        s.tangent_rhs(c["D"], c["dD"], c["CL"], c["CR"])
        r = s.solve_tangent(rtol=1e-13)
        dx = s.get_tangent()
    d = rel_l2(dx, c["dxd"])
    print(f"tangent against direct {nx}x{ny}: numpy CG {c['it_dx']} iterations d_ref {c['d_dx']:.3e}; GPU {r.iters} iterations "
          f"rel {r.rel_residual:.3e} d {d:.3e}")
    assert r.converged and np.all(dx[c["dec"]] == 0.0)
    assert d <= max(1e-10, 10 * c["d_dx"]), (d, c["d_dx"])


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_dot_product_on_the_device(pkg, nx, ny):
    """solve_cg(1e-13), field_jvp(dD), solve_adjoint(w) + field_vjp: <w', dx> against <g, d>, relative to |<w', dx>|.  Bar: 10 x
    the same figure from the models on numpy's CG fields at that rtol, and at least 1e-9."""
    c = direct_case(nx, ny)
    CL, CR, D = c["CL"], c["CR"], c["D"]
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        rx = s.solve_cg(rtol=1e-13)
        x = s.get_field()
        dx = s.field_jvp(D, c["dD"], CL, CR, rtol=1e-13)
        rl = s.solve_adjoint(c["w"], rtol=1e-13)
        g, _ = s.field_vjp(D, CL, CR)
        assert np.array_equal(s.get_field(), x) and np.array_equal(s.get_tangent(), dx)
    lhs, rhs = float(np.sum(c["wp"] * dx)), float(np.sum(g * c["d"]))
    rel = abs(lhs - rhs) / abs(lhs)
    print(f"tangent dot product {nx}x{ny}: <w', dx> {lhs:.9e} <g, d> {rhs:.9e} rel {rel:.3e}; numpy CG {c['dot_np']:.3e}")
    assert rx.converged and rl.converged
    assert rel <= max(1e-9, 10 * c["dot_np"]), (rel, c["dot_np"])


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_field_adjoint_tangent_and_maps_alone(pkg, oracle):
    nx, ny = 34, 20                                      # (even: a system with a wall link into the next row needs it)
    CL, CR = 0.0, 1.0
    x, D = make_case(nx, ny, 1, CL, CR, 3)
    x, D = x[0], D[0]
    dD = make_direction(D, 3)
    lam = np.random.default_rng(2).standard_normal((ny, nx))
    L = pkg._capi.load()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)      # noqa: E731
    res = (pkg._capi.CGResultC * 1)()
    with pkg.Solver(nx, ny) as s:
        _refused(pkg, s.device_tangent_rhs_ptr, -5)      # DEFF_ESTATE: no map yet
        _refused(pkg, s.get_tangent, -5)
        _refused(pkg, s.device_tangent_ptr, -5)
        _refused(pkg, lambda: s.tangent_rhs(D, dD, CL, CR), -5, "no field")
        _refused(pkg, s.device_tangent_rhs_ptr, -5)
        s.set_field(x)
        s.tangent_rhs(D, dD, CL, CR)                     # the pass needs no system ...
        _refused(pkg, s.solve_tangent, -5, "no system")  # ... the solve does
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.set_field(x)
        _refused(pkg, s.solve_tangent, -5, "right-hand side")           # before any pass
        r0, n0 = s.tangent_rhs(D, dD, CL, CR)
        r1, _ = s.tangent_rhs(D, dD, 1.0, 1.0)           # CR == CL is allowed
        assert np.all(np.isfinite(r1))
        s.tangent_rhs(D, dD, CL, CR)
        assert s.solve_tangent(rtol=1e-10).converged
        dx0 = s.get_tangent()
        s.set_adjoint(lam)
        s.field_vjp(D, CL, CR)
        pr, pitch = s.device_tangent_rhs_ptr()
        pv, _ = s.device_field_vjp_ptr()
        dev_r, dev_v = device_rows(pr, ny, pitch), device_rows(pv, ny, pitch)
        assert np.array_equal(dev_r[:, :nx], r0)

        def unchanged(tangent=True):
            assert s.device_tangent_rhs_ptr() == (pr, pitch) and np.array_equal(device_rows(pr, ny, pitch), dev_r)
            assert np.array_equal(device_rows(pv, ny, pitch), dev_v)
            assert np.array_equal(s.get_field(), x)
            assert np.array_equal(s.get_adjoint(), lam)
            if tangent:
                assert np.array_equal(s.get_tangent(), dx0)

        # NULL arguments
        assert L.deff_tangent_rhs_D(s._ctx, None, vp(dD), CL, CR, None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        assert L.deff_tangent_rhs_D(s._ctx, vp(D), None, CL, CR, None, None, None) == -1 and b"dD is NULL" in L.deff_last_error()
        assert L.deff_solve_tangent(s._ctx, 1e-10, 100, 64, None) == -1
        assert L.deff_get_tangent(s._ctx, None) == -1
        assert L.deff_device_tangent(s._ctx, None, None) == -1
        assert L.deff_device_tangent_rhs(s._ctx, None, None) == -1
        unchanged()
        for rtol, mi, ce in ((-1.0, 100, 64), (float("nan"), 100, 64), (float("inf"), 100, 64), (1e-10, -1, 64), (1e-10, 100, 0)):
            _refused(pkg, lambda: s.solve_tangent(rtol=rtol, max_iter=mi, check_every=ce), -1)
            unchanged()
        # r and norm2 may each be NULL
        assert L.deff_tangent_rhs_D(s._ctx, vp(D), vp(dD), CL, CR, None, None, None) == 0
        unchanged()
        # a wall link into the neighbouring row: explicit-only.  A new system: the tangent and the map's use are the old one's
        A, b = s.get_system()
        A3 = A.copy()
        A3[2 * nx, 1] = -0.5
        s.set_system(A3, b, D, CL, CR)
        _refused(pkg, s.get_tangent, -5)
        _refused(pkg, s.device_tangent_ptr, -5)
        s.set_adjoint(lam)
        s.tangent_rhs(D, dD, CL, CR)
        _refused(pkg, s.solve_tangent, -1, "wall column")
        _refused(pkg, s.get_tangent, -5)
        unchanged(tangent=False)
        # a system that is not symmetric: the verdict on the device comes before dx is touched
        s.set_system(A, b, D, CL, CR)
        s.set_adjoint(lam)
        s.tangent_rhs(D, dD, CL, CR)
        assert s.solve_tangent(rtol=1e-10).converged and np.array_equal(s.get_tangent(), dx0)
        A2 = A.copy()
        i, j = np.argwhere((D[:, :-1] != 0.0) & (D[:, 1:] != 0.0))[40]
        A2[i * nx + j, 2] *= 2.0                         # an E link that differs from its partner's W link
        s.set_system(A2, b, D, CL, CR)
        s.set_adjoint(lam)
        s.tangent_rhs(D, dD, CL, CR)
        _refused(pkg, s.solve_tangent, -1, "symmetric")
        unchanged(tangent=False)
        # every call that replaces the system or the image invalidates the tangent and the map's use as a right-hand side
        s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        for again in (lambda: s.assemble_2phase(1e-3, 1.0, CL, CR), lambda: s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR),
                      lambda: s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR), lambda: s.assemble_from_D(D, CL, CR),
                      lambda: s.set_system(A, b, D, CL, CR), lambda: s.synth_image(1, 0),
                      lambda: s.set_image(oracle.synth_mask(nx, ny, 12345, 0))):
            s.assemble_from_D(D, CL, CR)
            s.set_field(x)
            s.tangent_rhs(D, dD, CL, CR)
            assert s.solve_tangent(rtol=1e-10).converged and np.array_equal(s.get_tangent(), dx0)
            again()
            _refused(pkg, s.get_tangent, -5)
            _refused(pkg, s.device_tangent_ptr, -5)
            _refused(pkg, s.solve_tangent, -5)
            assert s.device_tangent_rhs_ptr() == (pr, pitch) and np.array_equal(device_rows(pr, ny, pitch), dev_r)
        # r = 0 (the direction 0): at once, dx = 0
        s.assemble_from_D(D, CL, CR)
        s.set_field(x)
        _, n2 = s.tangent_rhs(D, np.zeros((ny, nx)), CL, CR)
        q = s.solve_tangent()
        assert n2 == 0.0 and (q.iters, q.rel_residual, q.converged, q.deff_raw) == (0, 0.0, True, 0.0)
        assert not s.get_tangent().any()
        assert np.array_equal(s.get_field(), x)
    with pkg.SlabRank(nx, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        sr.assemble_2phase(1e-3, 1.0, CL, CR)
        sr.init_linear(CL, CR)
        x0 = sr.get_field()
        out = np.zeros((ny, nx))
        one = np.ones((ny, nx))
        assert L.deff_tangent_rhs_D(sr._ctx, vp(one), vp(one), CL, CR, vp(out), None, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert L.deff_solve_tangent(sr._ctx, 1e-10, 100, 64, res) == -1 and b"row-slab" in L.deff_last_error()
        assert L.deff_get_tangent(sr._ctx, vp(out)) == -1 and b"row-slab" in L.deff_last_error()
        p = C.c_void_p()
        assert L.deff_device_tangent(sr._ctx, C.byref(p), None) == -1 and b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0) and np.all(out == 0.0)


# ---- torch ---------------------------------------------------------------------------------------------------------------

def test_torch_forward_mode(pkg, oracle):
    """torch.autograd.forward_ad at 12 x 9 on cpu and cuda and on a stack of 2 on a passed solver.  concentration_field: the
    tangent against the model on the direct solves (bar: max(1e-10, 10 x numpy CG's own distance at the op's rtol)).
    effective_diffusivity: the tangent equals (g * tD).sum() of the gradient map backward returns, and matches central
    differences of the direct solve's Deff along tD (bar: 10 x the gap between the steps 1e-5 and 1e-6, as on the host).
    backward's results are what they are on Functions without the jvp methods."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from effectivediffusivityfvm_amd import concentration_field, effective_diffusivity
    nx, ny = 12, 9
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(12)
    Dn = np.exp(2.0 * rng.standard_normal((2, ny, nx)))
    tn = Dn * rng.standard_normal((2, ny, nx))
    wn = rng.standard_normal((2, ny, nx))
    zero = np.zeros((ny, nx))
    refs = []
    for k in range(2):
        A, b = oracle.discretize(Dn[k], CL, CR)
        xd = block_thomas(A, b, nx, ny)
        dxd = block_thomas(A, model(xd, Dn[k], tn[k], CL, CR)[0].ravel(), nx, ny)
        tx = pcg_numpy(A, b, oracle.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-12)
        tdx = pcg_numpy(A, model(tx.x, Dn[k], tn[k], CL, CR)[0].ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-12)
        refs.append((dxd, rel_l2(tdx.x, dxd)))

    def deff(Dq):
        Aq, bq = oracle.discretize(Dq, CL, CR)
        return oracle.flux_deff(block_thomas(Aq, bq, nx, ny), Dq, CL, CR)[0]

    fd5 = (deff(Dn[0] + 1e-5 * tn[0]) - deff(Dn[0] - 1e-5 * tn[0])) / 2e-5
    fd6 = (deff(Dn[0] + 1e-6 * tn[0]) - deff(Dn[0] - 1e-6 * tn[0])) / 2e-6
    for dev in ("cpu", "cuda"):
        D = torch.tensor(Dn[0], dtype=torch.float64, device=dev)
        t = torch.tensor(tn[0], dtype=torch.float64, device=dev)
        with fwAD.dual_level():
            x, dx = fwAD.unpack_dual(concentration_field(fwAD.make_dual(D, t), CL, CR))
            e, de = fwAD.unpack_dual(effective_diffusivity(fwAD.make_dual(D, t), CL, CR))
        assert dx.shape == D.shape and dx.device == D.device and dx.dtype == torch.float64
        d = rel_l2(dx.cpu().numpy(), refs[0][0])
        print(f"concentration_field jvp on {dev}: {d:.3e} from the model on the direct solves (numpy CG {refs[0][1]:.3e})")
        assert d <= max(1e-10, 10 * refs[0][1]), (d, refs[0][1])
        Dg = D.clone().requires_grad_(True)
        effective_diffusivity(Dg, CL, CR).backward()
        assert de.shape == () and de.device == D.device and torch.equal(de, (Dg.grad * t).sum((-2, -1)))
        gap, err = abs(fd5 - fd6) / abs(fd5), abs(float(de) - fd5) / abs(fd5)
        print(f"effective_diffusivity jvp on {dev}: {float(de):.9e}, central differences {fd5:.9e}: gap {gap:.3e} err {err:.3e}")
        assert gap < 1e-4, gap
        assert err <= 10.0 * gap, (err, gap)
    # a stack of 2 on a solver that is passed in and stays open
    D = torch.tensor(Dn, dtype=torch.float64, device="cuda")
    t = torch.tensor(tn, dtype=torch.float64, device="cuda")
    with pkg.Solver(nx, ny, nimg=2) as s:
        with fwAD.dual_level():
            dx = fwAD.unpack_dual(concentration_field(fwAD.make_dual(D, t), CL, CR, solver=s)).tangent
            de = fwAD.unpack_dual(effective_diffusivity(fwAD.make_dual(D, t), CL, CR, solver=s)).tangent
        s.init_linear(CL, CR)                            # the passed solver is still open
        Dg = D.clone().requires_grad_(True)
        effective_diffusivity(Dg, CL, CR, solver=s).sum().backward()
    assert dx.shape == (2, ny, nx) and de.shape == (2,)
    assert torch.equal(de, (Dg.grad * t).sum((-2, -1)))
    for k in range(2):
        d = rel_l2(dx[k].cpu().numpy(), refs[k][0])
        assert d <= max(1e-10, 10 * refs[k][1]), (k, d, refs[k][1])
    # backward is bitwise what the ops did before they had a jvp: the library calls of their two passes, made by hand
    w = torch.tensor(wn[0], dtype=torch.float64, device="cuda")
    Dg = torch.tensor(Dn[0], dtype=torch.float64, device="cuda", requires_grad=True)
    effective_diffusivity(Dg, CL, CR).backward()
    Dx = torch.tensor(Dn[0], dtype=torch.float64, device="cuda", requires_grad=True)
    (concentration_field(Dx, CL, CR) * w).sum().backward()
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(Dn[0], CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        assert s.solve_cg(rtol=1e-12).converged
        g_e, _ = s.sensitivity(Dn[0], CL, CR)
        xs = s.get_field()
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(Dn[0], CL, CR)
        s.set_field(xs)
        assert s.solve_adjoint(wn[0], rtol=1e-12).converged
        g_x, _ = s.field_vjp(Dn[0], CL, CR)
    assert np.array_equal(Dg.grad.cpu().numpy(), g_e) and np.array_equal(Dx.grad.cpu().numpy(), g_x)
