"""The field adjoint on the GPU (deff_solve_adjoint, deff_field_vjp_D, csrc/kernels_vjp.hpp): the pass bit for bit against the
numpy model of the normative expressions at every strip / seam / pad shape, the adjoint solve bit for bit against a twin context
that solves the same system as a forward one, against the direct solve, end to end on converged fields, what the calls leave
alone, refusals and the torch op."""
import ctypes as C
import functools

import numpy as np
import pytest

from field_vjp_model import field_vjp as model
from test_cg_host import block_thomas, decoupled_of, pcg_numpy, rel_l2
from test_field_vjp_host import central_fd
from test_gpu_sensitivity import _refused, device_rows, make_case

pytestmark = pytest.mark.gpu

WALLS = [(0.0, 1.0), (2.0, -1.0)]


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_lambda(nx, ny, nimg, seed):
    """A smooth-plus-random adjoint field (the map is a function of any x and lambda)."""
    rng = np.random.default_rng(seed + 77)
    j = (np.arange(nx) + 0.5) / nx
    i = (np.arange(ny) + 0.5) / ny
    lam = np.sin(np.pi * j)[None, None, :] * (1.0 + 0.3 * np.cos(2.0 * i))[None, :, None]
    return lam + 0.05 * rng.standard_normal((nimg, ny, nx))


# ---- the pass, bit for bit ----------------------------------------------------------------------------------------------

def check_map(pkg, nx, ny, nimg, CL, CR, kt=0, seed=0):
    """The map equals the model's (array_equal), the Euler sums are within 1e-13 sum|D g| of the model's long-double sums and
    the same bits on a second call; get_adjoint returns what set_adjoint took.  Returns (vjp_kt, vjp_items) as used."""
    x, D = make_case(nx, ny, nimg, CL, CR, seed)
    lam = make_lambda(nx, ny, nimg, seed)
    out = [model(x[k], lam[k], D[k], CL, CR) for k in range(nimg)]
    want, euler_want = np.stack([g for g, _ in out]), [e for _, e in out]
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_field(x.reshape(nimg * ny, nx))
        s.set_adjoint(lam.reshape(nimg * ny, nx))
        if kt:
            s.set_tuning("vjp_kt", kt)
        g, e = s.field_vjp(D.reshape(nimg * ny, nx), CL, CR)
        g2, e2 = s.field_vjp(D.reshape(nimg * ny, nx), CL, CR)
        plan = s.plan_value("vjp_kt"), s.plan_value("vjp_items")
        assert np.array_equal(s.get_adjoint(), lam.reshape(nimg * ny, nx))
        assert s.device_adjoint_ptr()[1] == s.device_field_ptr()[1] == 8 * (nx + (nx & 1))
        assert np.array_equal(s.get_field(), x.reshape(nimg * ny, nx))
    g, g2 = g.reshape(nimg, ny, nx), g2.reshape(nimg, ny, nx)
    e, e2 = np.atleast_1d(e), np.atleast_1d(e2)
    for k in range(nimg):
        bad = np.argwhere(g[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), g[k][tuple(bad[0])], want[k][tuple(bad[0])])
        size = float(np.sum(np.abs(D[k] * want[k])))
        rel = abs(float(np.longdouble(e[k]) - euler_want[k])) / size
        print(f"field vjp {nimg} x {nx}x{ny} kt {plan[0]} image {k}: euler {e[k]:.6e}, off the model's by {rel:.3e} of sum|D g|")
        assert rel <= 1e-13, (k, e[k], euler_want[k])
    assert np.array_equal(g, g2) and np.array_equal(e, e2)
    assert np.all(g[D == 0.0] == 0.0) and np.any(g != 0.0)
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
    """"vjp_kt": 9 tile rows, 2 strips -- kt = 1 has a seam every 8 rows (9 items per strip), kt = 2 every 16 (5 items, the last
    one 7 rows short), kt = 64 is clipped to the image (one item per strip, no seam)."""
    used, items = check_map(pkg, nx, ny, nimg, 0.0, 1.0, kt=kt, seed=7 + kt)
    assert (used, items) == {1: (1, 18), 2: (2, 10), 64: (9, 2)}[kt]


def test_map_matches_model_large(pkg):
    """2050 x 1537: 17 strips (the last one 2 columns wide), 193 tile rows, an odd height."""
    kt, items = check_map(pkg, 2050, 1537, 1, 0.0, 1.0, seed=99)
    assert items == 17 * ((193 + kt - 1) // kt)


# ---- the adjoint solve, bit for bit, against a twin context ---------------------------------------------------------------

@pytest.mark.parametrize("nimg,nx,ny", [(1, 130, 71), (1, 33, 40), (3, 33, 20)])
def test_adjoint_solve_equals_twin_forward_solve(pkg, nimg, nx, ny):
    """Context A solves A lambda = w beside its own system; context B is given A's matrix with w' (w zeroed at the rows A's
    forward system decouples) as its right-hand side and solves it as a forward system on the coefficient planes from x = 0.
    The same bits, iterations and residual -- under cg_fold and for every check_every."""
    CL, CR = 2.0, -1.0
    rng = np.random.default_rng(nimg * 1000 + nx)
    _, D = make_case(nx, ny, nimg, CL, CR, nx + ny)
    D2 = D.reshape(nimg * ny, nx)
    w = rng.standard_normal((nimg * ny, nx))
    with pkg.Solver(nx, ny, nimg=nimg) as a, pkg.Solver(nx, ny, nimg=nimg) as b:
        a.assemble_from_D(D2, CL, CR)
        Am, bm = a.get_system()
        dec = decoupled_of(Am, bm).reshape(nimg * ny, nx)
        assert dec.any() and np.all(dec[D2 == 0.0])
        wp = np.where(dec, 0.0, w)
        b.set_system(Am, wp.ravel(), D2, CL, CR)
        b.set_tuning("cg_planes", 2)
        b.set_field(np.zeros((nimg * ny, nx)))
        rb = b.solve_cg(rtol=1e-11)
        xb = b.get_field()
        rb = rb if isinstance(rb, list) else [rb]
        assert all(r.converged and r.iters > 10 for r in rb), rb
        for fold, every in ((0, 64), (1, 64), (0, 1), (0, 7)):
            a.set_tuning("cg_fold", fold)
            ra = a.solve_adjoint(w, rtol=1e-11, check_every=every)
            ra = ra if isinstance(ra, list) else [ra]
            lam = a.get_adjoint()
            assert a.plan_value("cg_impl") == 3 and a.plan_value("cg_fold") == fold
            bad = np.argwhere(lam != xb)
            assert bad.size == 0, (fold, every, len(bad), bad[:5].tolist())
            assert np.all(lam[dec] == 0.0)
            for k in range(nimg):
                assert (ra[k].iters, ra[k].rel_residual, ra[k].converged) == (rb[k].iters, rb[k].rel_residual, rb[k].converged)
                assert ra[k].deff_raw == 0.0 and ra[k].loop_ms > 0.0
        print(f"adjoint twin {nimg} x {nx}x{ny}: {[r.iters for r in rb]} iterations, rel {[r.rel_residual for r in rb]}")


def _twin_solve(pkg, nx, ny, A, wp, D, CL, CR, **kw):
    """A fresh one-image context that solves A lambda = w' as a forward system on the planes from a zero field, unfolded ->
    ((iters, rel_residual, converged), field)."""
    with pkg.Solver(nx, ny) as b:
        b.set_system(A, np.ascontiguousarray(wp).ravel(), D, CL, CR)
        b.set_tuning("cg_planes", 2)
        b.set_field(np.zeros((ny, nx)))
        r = b.solve_cg(**kw)
        assert b.plan_value("cg_impl") == 3 and b.plan_value("cg_fold") == 0
        return (r.iters, r.rel_residual, r.converged), b.get_field()


def test_adjoint_solve_on_a_stack_with_images_that_have_nothing_to_solve(pkg):
    """"An image with ||w'|| = 0 returns at once" while the others iterate: on a stack of 3, image 1 has w = 0 and image 2 has
    w != 0 only where the forward system decouples the cell (so w' = 0 although w is not).  Both report iters 0, residual 0,
    converged, lambda = 0; image 0 is solved as if it were alone -- its twin's bits -- under cg_fold 0 and 1."""
    nimg, nx, ny = 3, 33, 20
    CL, CR = 2.0, -1.0
    rng = np.random.default_rng(33203)
    _, D = make_case(nx, ny, nimg, CL, CR, 5)
    D2 = D.reshape(nimg * ny, nx)
    with pkg.Solver(nx, ny, nimg=nimg) as a:
        a.assemble_from_D(D2, CL, CR)
        Am, bm = a.get_system()
        dec = decoupled_of(Am, bm).reshape(nimg, ny, nx)
        assert dec[2].any() and not dec[2].all()
        w = np.zeros((nimg, ny, nx))
        w[0] = rng.standard_normal((ny, nx))
        w[2][dec[2]] = rng.standard_normal(int(dec[2].sum())) + 3.0
        assert w[2].any()
        n = nx * ny
        want, twin = _twin_solve(pkg, nx, ny, Am[:n], np.where(dec[0], 0.0, w[0]), D[0], CL, CR, rtol=1e-11)
        assert want[2] and want[0] > 10, want
        for fold in (0, 1):
            a.set_adjoint(np.ones((nimg * ny, nx)))          # (whatever lambda was before, a finished image holds 0)
            a.set_tuning("cg_fold", fold)
            r = a.solve_adjoint(w.reshape(nimg * ny, nx), rtol=1e-11)
            lam = a.get_adjoint().reshape(nimg, ny, nx)
            assert a.plan_value("cg_fold") == fold
            for k in (1, 2):
                assert (r[k].iters, r[k].rel_residual, r[k].converged, r[k].deff_raw) == (0, 0.0, True, 0.0), (fold, k, r[k].iters)
                assert not lam[k].any(), (fold, k)
            assert (r[0].iters, r[0].rel_residual, r[0].converged) == want, (fold, r[0].iters, r[0].rel_residual, want)
            bad = np.argwhere(lam[0] != twin)
            assert bad.size == 0, (fold, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("max_iter", [0, 3])
@pytest.mark.parametrize("nimg,nx,ny", [(1, 130, 71), (3, 33, 20)])
def test_a_partial_lambda_is_the_twins_and_valid(pkg, nimg, nx, ny, max_iter):
    """max_iter 0 and 3: lambda is what that many iterations leave -- the twin's bits, iterations and residual, image by image
    --, it is not converged, and it is valid all the same: deff_get_adjoint returns it and deff_field_vjp_D takes it (the
    model's map of the field and that lambda)."""
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + max_iter)
    x, D = make_case(nx, ny, nimg, CL, CR, nx)
    D2 = D.reshape(nimg * ny, nx)
    w = rng.standard_normal((nimg, ny, nx))
    n = nx * ny
    with pkg.Solver(nx, ny, nimg=nimg) as a:
        a.assemble_from_D(D2, CL, CR)
        a.set_field(x.reshape(nimg * ny, nx))
        Am, bm = a.get_system()
        dec = decoupled_of(Am, bm).reshape(nimg, ny, nx)
        r = a.solve_adjoint(w.reshape(nimg * ny, nx), rtol=1e-11, max_iter=max_iter)
        r = r if isinstance(r, list) else [r]
        lam = a.get_adjoint().reshape(nimg, ny, nx)
        g, _ = a.field_vjp(D2, CL, CR)
        g = g.reshape(nimg, ny, nx)
        assert np.array_equal(a.get_adjoint().reshape(nimg, ny, nx), lam)
        for k in range(nimg):
            want, twin = _twin_solve(pkg, nx, ny, Am[k * n:(k + 1) * n], np.where(dec[k], 0.0, w[k]), D[k], CL, CR, rtol=1e-11,
                                     max_iter=max_iter)
            assert (r[k].iters, r[k].rel_residual, r[k].converged) == want, (k, r[k].iters, r[k].rel_residual, want)
            assert r[k].iters == max_iter and not r[k].converged and r[k].rel_residual > 1e-11, (k, r[k].iters, r[k].rel_residual)
            assert np.array_equal(lam[k], twin), k
            assert lam[k].any() == (max_iter > 0)
            assert np.array_equal(g[k], model(x[k], lam[k], D[k], CL, CR)[0]), k


@pytest.mark.parametrize("nx,ny", [(130, 71), (33, 20)])
def test_an_active_row_without_links_counts(pkg, oracle, nx, ny):
    """The forward system decides which cells are decoupled: four zero links AND b == 0.  A cell of a caller's system with four
    zero links, A0 > 0 and b != 0 (its neighbours' links to it 0 as well: the matrix stays symmetric) is active, so its w
    counts: lambda there solves its own row, A0 lambda = w, and the whole lambda meets the honest-residual bar of
    test_gpu_cg.py::assert_honest.  Bar of the one row: its residual is one entry of r, so |w - A0 lambda| <= ||r|| <= that bar
    times ||w'||."""
    from test_cg_host import residual_np
    CL, CR = 0.0, 1.0
    rtol = 1e-11
    rng = np.random.default_rng(nx)
    D = np.exp(rng.standard_normal((ny, nx)))
    A, b = oracle.discretize(D, CL, CR)
    A = A.copy().reshape(ny, nx, 5)                          # P, W, E, S (row + 1), N (row - 1)
    b = b.copy().reshape(ny, nx)
    i, j = ny // 2, 128 if nx > 129 else nx // 2             # (column 128: its W neighbour lies across a 128-column seam)
    A[i, j] = (2.5, 0.0, 0.0, 0.0, 0.0)
    b[i, j] = 0.75
    A[i, j - 1, 2] = A[i, j + 1, 1] = A[i - 1, j, 3] = A[i + 1, j, 4] = 0.0
    A, b = A.reshape(-1, 5), b.ravel()
    dec = decoupled_of(A, b).reshape(ny, nx)
    assert not dec.any()
    w = rng.standard_normal((ny, nx))
    with pkg.Solver(nx, ny) as s:
        s.set_system(A, b, D, CL, CR)
        r = s.solve_adjoint(w, rtol=rtol)
        lam = s.get_adjoint()
    bar = rtol * (1 + 1e-6) + 1e-13
    rn = residual_np(A, w.ravel(), lam, nx, ny)
    own = abs(w[i, j] - 2.5 * lam[i, j]) / float(np.sqrt(np.sum(w * w)))
    print(f"active row without links {nx}x{ny}: {r.iters} iterations, rel {r.rel_residual:.3e}, host {rn:.3e}, own row {own:.3e}")
    assert r.converged and r.iters > 10
    assert rn <= bar, rn
    assert lam[i, j] != 0.0 and own <= bar, (lam[i, j], w[i, j] / 2.5, own)


def test_lifetime_across_streams(pkg, oracle):
    """deff_amd.h lists both streams among the calls that invalidate lambda, and a refused call changes nothing: on a stack of
    2, an accepted deff_solve_stream and an accepted deff_solve_cg_stream leave deff_get_adjoint, deff_device_adjoint and
    deff_field_vjp_D refused (DEFF_ESTATE); a deff_solve_cg_stream refused for Df = -1 and a deff_solve_stream refused under
    "prescaled" 1 on the explicit kernel leave lambda's bits, and its validity, as they were."""
    nimg, nx, ny = 2, 33, 20
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(2033)
    pix = [np.where(rng.random((ny, nx)) < 0.5, 0, 255).astype(np.uint8) for _ in range(nimg)]
    w = rng.standard_normal((nimg * ny, nx))
    lam0 = rng.standard_normal((nimg * ny, nx))
    Dp = np.exp(rng.standard_normal((nimg * ny, nx)))

    def invalid(s):
        _refused(pkg, s.get_adjoint, -5)
        _refused(pkg, s.device_adjoint_ptr, -5)
        _refused(pkg, lambda: s.field_vjp(Dp, CL, CR), -5, "adjoint")

    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_image(np.stack(pix))
        s.assemble_2phase(1e-2, 1.0, CL, CR)
        s.init_linear(CL, CR)
        s.set_adjoint(lam0)
        assert np.array_equal(s.get_adjoint(), lam0)
        res = s.solve_stream(pix + pix[:1], 1e-2, 1.0, CL, CR, 1e-2, 7, check_every=7)
        assert len(res) == 3
        invalid(s)
        r = s.solve_adjoint(w, rtol=1e-9)                    # on the system the stream left in the slots
        assert all(q.converged for q in r)
        res = s.solve_cg_stream(pix + pix[:1], 1e-2, 1.0, CL, CR, rtol=1e-6, max_iter=100000)
        assert len(res) == 3
        invalid(s)
        r = s.solve_adjoint(w, rtol=1e-9)
        assert all(q.converged and q.iters > 0 for q in r)
        lam = s.get_adjoint()
        x = s.get_field()
        g0, e0 = s.field_vjp(Dp, CL, CR)
        with pytest.raises(pkg.DeffError) as e:
            s.solve_cg_stream(pix, 1e-2, -1.0, CL, CR, rtol=1e-6, max_iter=10)
        assert e.value.code == -1 and "admissible" in str(e.value), str(e.value)
        assert np.array_equal(s.get_adjoint(), lam) and np.array_equal(s.get_field(), x)
        s.set_kernel("explicit")
        s.set_tuning("prescaled", 1)
        with pytest.raises(pkg.DeffError) as e:
            s.solve_stream(pix, 1e-2, 1.0, CL, CR, 1e-2, 7, check_every=7)
        assert e.value.code == -1 and "prescaled" in str(e.value), str(e.value)
        assert np.array_equal(s.get_adjoint(), lam) and np.array_equal(s.get_field(), x)
        p, pitch = s.device_adjoint_ptr()
        dev = device_rows(p, nimg * ny, pitch)
        assert pitch == 8 * (nx + 1) and np.array_equal(dev[:, :nx], lam) and np.all(dev[:, nx] == 0.0)
        g1, e1 = s.field_vjp(Dp, CL, CR)
        assert np.array_equal(g1, g0) and np.array_equal(e1, e0)


# ---- against the direct solves, and end to end ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def direct_case(nx, ny):
    """One system per shape, shared and left unchanged: D = exp(2 N(0, 1)) with zero cells, w = N(0, 1); the direct solves
    x = A^-1 b and lambda = A^-1 w' (decoupled cells fixed at 0), the model's map on them, and what numpy's float64 CG stopped at
    rtol 1e-13 leaves of each: the reference's own error, which sets the bars."""
    import oracle_binding as ob
    ob.build()
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    D[rng.random((ny, nx)) < 0.03] = 0.0
    D[ny // 2, nx // 2 - 1:nx // 2 + 1] = 0.0
    D[3, 0] = 0.0
    w = rng.standard_normal((ny, nx))
    A, b = ob.discretize(D, CL, CR)
    dec = decoupled_of(A, b)
    wp = np.where(dec.reshape(ny, nx), 0.0, w)
    xd = block_thomas(A, b, nx, ny, fixed=dec)
    ld = block_thomas(A, wp.ravel(), nx, ny, fixed=dec)
    g_ref, _ = model(xd, ld, D, CL, CR)
    tx = pcg_numpy(A, b, ob.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-13)
    tl = pcg_numpy(A, wp.ravel(), np.zeros((ny, nx)), nx, ny, 50_000, np.float64, rtol=1e-13)
    g_np, euler_np = model(tx.x, tl.x, D, CL, CR)
    out = dict(CL=CL, CR=CR, D=D, w=w, dec=dec.reshape(ny, nx), xd=xd, ld=ld, g_ref=g_ref,
               d_lam=rel_l2(tl.x, ld), d_g=rel_l2(g_np, g_ref),
               e_np=abs(float(euler_np)) / float(np.sum(np.abs(D * g_np))), it_x=tx.iters, it_l=tl.iters)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_adjoint_solve_against_direct_solve(pkg, nx, ny):
    """lambda at rtol 1e-13 against block_thomas(A, w', fixed = decoupled).  Bar as for fields in test_gpu_sensitivity.py:
    max(1e-10, 10 d_ref), d_ref the same distance for numpy's float64 CG stopped at the same rtol."""
    c = direct_case(nx, ny)
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(c["D"], c["CL"], c["CR"])
        r = s.solve_adjoint(c["w"], rtol=1e-13)
        lam = s.get_adjoint()
    d = rel_l2(lam, c["ld"])
    print(f"adjoint against direct {nx}x{ny}: numpy CG {c['it_l']} iterations d_ref {c['d_lam']:.3e}; GPU {r.iters} iterations "
          f"rel {r.rel_residual:.3e} d {d:.3e}")
    assert r.converged and np.all(lam[c["dec"]] == 0.0)
    assert d <= max(1e-10, 10 * c["d_lam"]), (d, c["d_lam"])


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_end_to_end_against_direct_solves(pkg, nx, ny):
    """assemble_from_D + solve_cg(1e-13) + solve_adjoint(w, 1e-13) + field_vjp against the model on the two direct solves, under
    the same rule; the Euler sum within 1e-9 sum|D g|, and within 10 x what the model leaves on numpy's CG fields at that rtol."""
    c = direct_case(nx, ny)
    CL, CR, D = c["CL"], c["CR"], c["D"]
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        rx = s.solve_cg(rtol=1e-13)
        x = s.get_field()
        rl = s.solve_adjoint(c["w"], rtol=1e-13)
        assert np.array_equal(s.get_field(), x)
        g, e = s.field_vjp(D, CL, CR)
    d = rel_l2(g, c["g_ref"])
    e_rel = abs(e) / float(np.sum(np.abs(D * g)))
    print(f"field vjp end to end {nx}x{ny}: numpy CG {c['it_x']} + {c['it_l']} iterations d_ref {c['d_g']:.3e} euler {c['e_np']:.3e}; "
          f"GPU {rx.iters} + {rl.iters} iterations d {d:.3e} euler {e_rel:.3e}")
    assert rx.converged and rl.converged
    assert d <= max(1e-10, 10 * c["d_g"]), (d, c["d_g"])
    assert e_rel <= 1e-9, e_rel
    assert e_rel <= 10 * c["e_np"], (e_rel, c["e_np"])


# ---- what the calls leave alone --------------------------------------------------------------------------------------

def _image_context(pkg, oracle, nx, ny, native3=False, **kw):
    s = pkg.Solver(nx, ny, **kw)
    s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
    if native3:
        s.assemble_3phase_native(1e-3, 1.0, 10.0, 0.0, 1.0)
    else:
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
    s.init_linear(0.0, 1.0)
    return s


def test_state_is_left_alone(pkg, oracle):
    """After solve_adjoint and field_vjp the field, get_system, the dictionary and the sensitivity map are what they were, and
    a following solve_cg gives a fresh context's bits, on the row table and on the planes."""
    nx, ny = 67, 40                                      # odd width: a pad column
    rng = np.random.default_rng(8)
    w = rng.standard_normal((ny, nx))
    Dp = oracle.fill_D_2phase(oracle.synth_mask(nx, ny, 12345, 0), 1.0, 1e-3)
    for planes in (0, 2):
        with _image_context(pkg, oracle, nx, ny) as s, _image_context(pkg, oracle, nx, ny) as fresh:
            s.sweeps(5)
            fresh.sweeps(5)
            x0 = s.get_field()
            A0, b0 = s.get_system()
            rows0, codes0 = s.dictionary()
            s.sensitivity()
            p0, pitch = s.device_sensitivity_ptr()
            map0 = device_rows(p0, ny, pitch)
            r = s.solve_adjoint(w, rtol=1e-9)
            g, e = s.field_vjp(Dp, 0.0, 1.0)
            assert r.converged and s.plan_value("cg_impl") == 3 and np.all(np.isfinite(g))
            assert np.array_equal(s.get_field(), x0)
            A1, b1 = s.get_system()
            assert np.array_equal(A1, A0) and np.array_equal(b1, b0)
            rows1, codes1 = s.dictionary()
            assert np.array_equal(rows1, rows0) and np.array_equal(codes1, codes0)
            assert s.device_sensitivity_ptr() == (p0, pitch) and np.array_equal(device_rows(p0, ny, pitch), map0)
            pv, pitch_v = s.device_field_vjp_ptr()
            dev = device_rows(pv, ny, pitch_v)
            assert pitch_v == pitch and np.array_equal(dev[:, :nx], g) and np.all(dev[:, nx:] == 0.0)
            lam = s.get_adjoint()
            for c in (s, fresh):
                c.set_tuning("cg_planes", planes)
            r1, r2 = s.solve_cg(rtol=1e-10), fresh.solve_cg(rtol=1e-10)
            assert (r1.iters, r1.rel_residual, r1.deff_raw) == (r2.iters, r2.rel_residual, r2.deff_raw)
            assert np.array_equal(s.get_field(), fresh.get_field())
            assert s.plan_value("cg_impl") == fresh.plan_value("cg_impl") == (3 if planes else 1)
            assert lam.any() and np.array_equal(s.get_adjoint(), lam)        # lambda outlives a forward solve


@pytest.mark.parametrize("form", ["resident", "streaming"])
def test_no_side_effects_on_a_jacobi_run(pkg, oracle, form):
    """sweeps(27) + solve(...) with an adjoint solve and the pass in between give the bits they give without the calls."""
    nx, ny = 256, 192
    rng = np.random.default_rng(3)
    w = rng.standard_normal((ny, nx))
    runs = []
    for call in (False, True):
        with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
            if form == "streaming":
                s.set_tuning("tb_impl", 1)
            s.synth_image(12345, 0)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            s.sweeps(27)
            if call:
                s.solve_adjoint(w, rtol=1e-6, max_iter=128)
                g, e, ms = s.field_vjp(np.ones((ny, nx)), 0.0, 1.0, timing=True)
                assert np.all(np.isfinite(g)) and np.isfinite(e) and ms > 0.0
            r = s.solve(1e-9, 101, check_every=50)
            p = s.plan()
            assert p["tb_impl"] == (2 if form == "resident" else 1), p
            assert np.isfinite(r.loop_ms) and r.loop_ms > 0.0, r
            runs.append((s.get_field(), r.iters, r.checks, r.deff_raw, r.conv, s.plan_value("tb_fallbacks")))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1:] == runs[1][1:], (runs[0][1:], runs[1][1:])


@pytest.mark.parametrize("native3", [False, True])
def test_native_systems(pkg, oracle, native3):
    """A native 2-phase and a native 3-phase system: the planes are built from the image, the solve runs on them ("cg_impl" 3),
    the dictionary and "native3_rows" stay."""
    nx, ny = 66, 40
    rng = np.random.default_rng(4)
    w = rng.standard_normal((ny, nx))
    with _image_context(pkg, oracle, nx, ny, native3=native3) as s:
        rows0, codes0 = s.dictionary()
        n3 = s.plan_value("native3_rows")
        assert n3 == (452 if native3 else 0)
        A0, b0 = s.get_system()
    with _image_context(pkg, oracle, nx, ny, native3=native3) as s:
        r = s.solve_adjoint(w, rtol=1e-9)
        lam = s.get_adjoint()
        assert r.converged and r.iters > 0 and s.plan_value("cg_impl") == 3
        rows1, codes1 = s.dictionary()
        assert np.array_equal(rows1, rows0) and np.array_equal(codes1, codes0)
        assert s.plan_value("native3_rows") == n3
        dec = decoupled_of(A0, b0).reshape(ny, nx)
        assert np.all(lam[dec] == 0.0) and np.all(np.isfinite(lam)) and lam.any()
        # the residual of the returned lambda, recomputed on the host from the system the context exports
        from test_cg_host import residual_np
        wp = np.where(dec, 0.0, w)
        assert residual_np(A0, wp.ravel(), np.where(dec, 0.0, lam), nx, ny) <= 2e-9


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_field_adjoint_and_map_alone(pkg, oracle):
    nx, ny = 34, 20
    CL, CR = 0.0, 1.0
    x, D = make_case(nx, ny, 1, CL, CR, 3)
    x, D = x[0], D[0]
    lam = make_lambda(nx, ny, 1, 3)[0]
    w = np.random.default_rng(1).standard_normal((ny, nx))
    L = pkg._capi.load()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)      # noqa: E731
    res = (pkg._capi.CGResultC * 1)()
    with pkg.Solver(nx, ny) as s:
        _refused(pkg, s.device_field_vjp_ptr, -5)        # DEFF_ESTATE: no map yet
        _refused(pkg, s.get_adjoint, -5)
        _refused(pkg, s.device_adjoint_ptr, -5)
        _refused(pkg, lambda: s.solve_adjoint(w), -5, "no system")
        s.set_adjoint(lam)
        _refused(pkg, lambda: s.field_vjp(D, CL, CR), -5, "no field")
    with pkg.Solver(nx, ny) as s:
        s.set_field(x)
        _refused(pkg, lambda: s.field_vjp(D, CL, CR), -5, "adjoint")     # no lambda yet
        s.assemble_from_D(D, CL, CR)
        s.set_adjoint(lam)
        g0, e0 = s.field_vjp(D, CL, CR)
        g1, _ = s.field_vjp(D, 1.0, 1.0)                 # CR == CL is allowed
        assert np.all(np.isfinite(g1))
        s.field_vjp(D, CL, CR)
        p0, pitch = s.device_field_vjp_ptr()
        dev0 = device_rows(p0, ny, pitch)
        assert np.array_equal(dev0, g0)

        def unchanged():
            assert s.device_field_vjp_ptr() == (p0, pitch) and np.array_equal(device_rows(p0, ny, pitch), dev0)
            assert np.array_equal(s.get_field(), x)
            assert np.array_equal(s.get_adjoint(), lam)

        assert L.deff_field_vjp_D(s._ctx, None, CL, CR, None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        unchanged()
        assert L.deff_solve_adjoint(s._ctx, None, 1e-10, 100, 64, res) == -1
        assert L.deff_solve_adjoint(s._ctx, vp(w), 1e-10, 100, 64, None) == -1
        unchanged()
        for rtol, mi, ce in ((-1.0, 100, 64), (float("nan"), 100, 64), (float("inf"), 100, 64), (1e-10, -1, 64), (1e-10, 100, 0)):
            _refused(pkg, lambda: s.solve_adjoint(w, rtol=rtol, max_iter=mi, check_every=ce), -1)
            unchanged()
        # a system that is not symmetric: the verdict on the device comes before lambda is touched
        A, b = s.get_system()
        A2 = A.copy()
        i, j = np.argwhere((D[:, :-1] != 0.0) & (D[:, 1:] != 0.0))[40]
        assert A2[i * nx + j, 2] != 0.0
        A2[i * nx + j, 2] *= 2.0                         # an E link that differs from its partner's W link
        s.set_system(A2, b, D, CL, CR)
        _refused(pkg, s.get_adjoint, -5)                 # a new system: lambda was the old one's
        _refused(pkg, lambda: s.field_vjp(D, CL, CR), -5, "adjoint")
        s.set_adjoint(lam)
        _refused(pkg, lambda: s.solve_adjoint(w), -1, "symmetric")
        unchanged()
        # a wall link into the neighbouring row: explicit-only
        A3 = A.copy()
        A3[2 * nx, 1] = -0.5
        s.set_system(A3, b, D, CL, CR)
        s.set_adjoint(lam)
        _refused(pkg, lambda: s.solve_adjoint(w), -1, "wall column")
        unchanged()
        # every call that replaces the system or the image invalidates lambda
        s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        _refused(pkg, s.get_adjoint, -5)
        for again in (lambda: s.assemble_2phase(1e-3, 1.0, CL, CR), lambda: s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR),
                      lambda: s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR), lambda: s.assemble_from_D(D, CL, CR),
                      lambda: s.synth_image(1, 0)):
            s.set_adjoint(lam)
            again()
            _refused(pkg, s.device_adjoint_ptr, -5)
            _refused(pkg, lambda: s.field_vjp(D, CL, CR), -5, "adjoint")
        assert np.array_equal(device_rows(p0, ny, pitch), dev0)
        # g and euler may each be NULL
        s.assemble_from_D(D, CL, CR)
        s.set_adjoint(lam)
        assert L.deff_field_vjp_D(s._ctx, vp(D), CL, CR, None, None, None) == 0
        assert np.array_equal(device_rows(s.device_field_vjp_ptr()[0], ny, pitch), dev0)
        # w = 0: at once, lambda = 0
        r = s.solve_adjoint(np.zeros((ny, nx)))
        assert (r.iters, r.rel_residual, r.converged, r.deff_raw) == (0, 0.0, True, 0.0)
        assert not s.get_adjoint().any()
        assert np.array_equal(s.get_field(), x)
    with pkg.SlabRank(nx, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        sr.assemble_2phase(1e-3, 1.0, CL, CR)
        sr.init_linear(CL, CR)
        x0 = sr.get_field()
        out = np.zeros((ny, nx))
        assert L.deff_solve_adjoint(sr._ctx, vp(w), 1e-10, 100, 64, res) == -1 and b"row-slab" in L.deff_last_error()
        assert L.deff_set_adjoint(sr._ctx, vp(lam)) == -1 and b"row-slab" in L.deff_last_error()
        assert L.deff_field_vjp_D(sr._ctx, vp(np.ones((ny, nx))), CL, CR, vp(out), None, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0) and np.all(out == 0.0)


# ---- torch ---------------------------------------------------------------------------------------------------------------

def test_torch_op(pkg, oracle):
    """concentration_field at 12 x 9 on cpu and cuda and on a stack of 2: the gradient of sum(w * x) against the model on the
    direct solves (bar: max(1e-10, 10 x numpy CG's own distance at the op's rtol)), the gradient of sum((x - x_target)^2)
    against central differences (bar: 10 x the gap between the steps 1e-5 and 1e-6, as on the host)."""
    import torch
    from effectivediffusivityfvm_amd import concentration_field
    nx, ny = 12, 9
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(12)
    Dn = np.exp(2.0 * rng.standard_normal((2, ny, nx)))
    wn = rng.standard_normal((2, ny, nx))
    refs = []
    for k in range(2):
        A, b = oracle.discretize(Dn[k], CL, CR)
        xd = block_thomas(A, b, nx, ny)
        ld = block_thomas(A, wn[k].ravel(), nx, ny)
        g_ref, _ = model(xd, ld, Dn[k], CL, CR)
        tx = pcg_numpy(A, b, oracle.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-12)
        tl = pcg_numpy(A, wn[k].ravel(), np.zeros((ny, nx)), nx, ny, 50_000, np.float64, rtol=1e-12)
        refs.append((xd, g_ref, rel_l2(tx.x, xd), rel_l2(model(tx.x, tl.x, Dn[k], CL, CR)[0], g_ref)))
    for dev in ("cpu", "cuda"):
        D = torch.tensor(Dn[0], dtype=torch.float64, device=dev, requires_grad=True)
        x = concentration_field(D, CL, CR)
        assert x.shape == D.shape and x.device == D.device and x.dtype == torch.float64
        dx = rel_l2(x.detach().cpu().numpy(), refs[0][0])
        assert dx <= max(1e-10, 10 * refs[0][2]), (dx, refs[0][2])
        (x * torch.tensor(wn[0], dtype=torch.float64, device=dev)).sum().backward()
        assert D.grad.device == D.device and D.grad.shape == D.shape
        d = rel_l2(D.grad.cpu().numpy(), refs[0][1])
        print(f"concentration_field on {dev}: forward {dx:.3e}, backward {d:.3e} from the model on the direct solves "
              f"(numpy CG {refs[0][2]:.3e}, {refs[0][3]:.3e})")
        assert d <= max(1e-10, 10 * refs[0][3]), (d, refs[0][3])
    # a stack of 2 on a solver that is passed in and stays open
    D = torch.tensor(Dn, dtype=torch.float64, device="cuda", requires_grad=True)
    with pkg.Solver(nx, ny, nimg=2) as s:
        x = concentration_field(D, CL, CR, solver=s)
        assert x.shape == (2, ny, nx) and x.device == D.device
        s.init_linear(CL, CR)                            # whatever happens to the solver between the two passes
        (x * torch.tensor(wn, dtype=torch.float64, device="cuda")).sum().backward()
        s.init_linear(CL, CR)                            # the passed solver is still open
    grad = D.grad.cpu().numpy()
    for k in range(2):
        d = rel_l2(grad[k], refs[k][1])
        assert d <= max(1e-10, 10 * refs[k][3]), (k, d, refs[k][3])
    # a quadratic loss against central differences of the direct solve
    xt = refs[0][0] + 0.1 * rng.standard_normal((ny, nx))

    def loss(Dq):
        Aq, bq = oracle.discretize(Dq, CL, CR)
        return float(np.sum((block_thomas(Aq, bq, nx, ny) - xt) ** 2))

    fd5, fd6 = central_fd(loss, Dn[0], 1e-5), central_fd(loss, Dn[0], 1e-6)
    D = torch.tensor(Dn[0], dtype=torch.float64, device="cuda", requires_grad=True)
    ((concentration_field(D, CL, CR) - torch.tensor(xt, dtype=torch.float64, device="cuda")) ** 2).sum().backward()
    g = D.grad.cpu().numpy()
    scale = np.max(np.abs(g))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(g - fd5)) / scale
    print(f"concentration_field quadratic loss: gap {gap:.3e} err {err:.3e}")
    assert gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)
    with pytest.raises(RuntimeError, match="did not converge"):
        concentration_field(torch.tensor(Dn[0], dtype=torch.float64), CL, CR, max_iter=2)
