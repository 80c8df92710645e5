"""The flux field on the GPU (deff_flux_field, deff_flux_field_D, csrc/kernels_flux.hpp): the maps, the left wall and the section
sums bit for bit against the numpy model of the normative expressions (tests/flux_model.py) at every strip / pad / run shape,
stacks against one-image contexts, the image-system form, conservation on converged fields, what the call leaves alone, and
refusals.  Nothing here is wider than 258 columns."""
import numpy as np
import pytest

import flux_model as fm
from test_gpu_sensitivity import _refused, device_rows

pytestmark = pytest.mark.gpu

CL, CR = 0.25, 1.5
U = 2.0 ** -53


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_D(ny, nx, nimg=1, seed=0, zeros=0.10):
    """D per cell in [1e-3, 2], some cells 0 (one of them on each wall)."""
    rng = np.random.default_rng(seed + 1000 * ny + nx)
    D = rng.uniform(1e-3, 2.0, (nimg, ny, nx))
    D[rng.random((nimg, ny, nx)) < zeros] = 0.0
    if zeros:
        D[:, ny // 2, 0] = 0.0
        D[:, ny - 1, nx - 1] = 0.0
    return D


def swept(s, D, cl=CL, cr=CR, sweeps=5):
    """The context's field after `sweeps` Jacobi sweeps from the linear guess: not converged, fy != 0.  The sweeps run on the
    system of D with its zeros raised to 1e-3: a cell with D == 0 has an all-zero matrix row, which a Jacobi sweep (w / a0 of
    the reference's update) turns into NaN, and NaN compares unequal to itself.  The pass itself is given D with its zeros."""
    s.assemble_from_D(np.where(D == 0.0, 1e-3, D).reshape(-1, D.shape[-1]), cl, cr)
    s.init_linear(cl, cr)
    s.sweeps(sweeps)
    x = s.get_field().reshape(D.shape)
    assert np.all(np.isfinite(x))
    return x


def model_stack(x, D, cl, cr, kt):
    out = [fm.flux_field(x[k], D[k], cl, cr) for k in range(x.shape[0])]
    fx, fy, left = (np.stack([o[i] for o in out]) for i in range(3))
    Q = np.stack([fm.sections(fx[k], left[k], x.shape[1], kt) for k in range(x.shape[0])])
    return fx, fy, left, Q


def assert_same(got, want, what):
    got, want = np.asarray(got).reshape(np.shape(want)), np.asarray(want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check_maps(pkg, ny, nx, nimg=1, kt=0, cl=CL, cr=CR):
    """fx, fy, left and sections for the walls (cl, cr) equal the model's on the context's own swept field (swept between CL
    and CR whatever cl and cr are), twice.  Returns (ff, x, D, flux_kt)."""
    D = make_D(ny, nx, nimg)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        x = swept(s, D)
        if kt:
            s.set_tuning("flux_kt", kt)
        ff = s.flux_field(D.reshape(nimg * ny, nx), cl, cr)
        ff2 = s.flux_field(D.reshape(nimg * ny, nx), cl, cr)
        used, items = s.plan_value("flux_kt"), s.plan_value("flux_items")
        assert np.array_equal(s.get_field().reshape(x.shape), x)
        px, py, pitch = s.device_flux_field_ptrs()
        assert pitch == s.device_field_ptr()[1] == 8 * (nx + (nx & 1)) and px != py
        for p, m in ((px, ff.fx), (py, ff.fy)):
            dev = device_rows(p, nimg * ny, pitch)
            assert np.array_equal(dev[:, :nx], m.reshape(nimg * ny, nx)) and np.all(dev[:, nx:] == 0.0)
    assert used >= 1 and items == ((nx + 127) // 128) * (((ny + 7) // 8 + used - 1) // used)
    assert ff.left.shape == (nimg, ny) and ff.sections.shape == (nimg, nx + 1)
    assert ff.fx.shape == ff.fy.shape == ((ny, nx) if nimg == 1 else (nimg, ny, nx))
    want = model_stack(x, D, cl, cr, used)
    for name, g, g2, w in zip(("fx", "fy", "left", "sections"), ff, ff2, want):
        assert_same(g, w, (name, ny, nx, nimg, used))
        assert np.array_equal(g, g2), name                       # the same bits on a second call
    assert np.all(want[1][:, -1, :] == 0.0)                      # image boundaries carry no fy
    if ny > 2:                                                   # (at 2 x 2 the whole second row has D == 0)
        assert np.any(want[1] != 0.0) and np.any(want[0] != 0.0)
    return ff, x, D, used


@pytest.mark.parametrize("ny,nx", [(2, 2), (9, 7), (8, 128), (17, 129), (17, 130), (5, 258)])
def test_maps_match_model(pkg, ny, nx):
    """(9, 7): an odd width, the pad column, a partial tile; (8, 128): exactly one strip; (17, 129) and (17, 130): an edge strip
    of 1 and of 2 columns; (5, 258): three strips."""
    check_maps(pkg, ny, nx)


@pytest.mark.parametrize("kt", [0, 1, 2])
@pytest.mark.parametrize("ny,nx", [(33, 40), (65, 130)])
def test_maps_match_model_at_runs(pkg, ny, nx, kt):
    """"flux_kt": items that start inside an image, a last run shorter than the others, several chunk partials per section."""
    _, _, _, used = check_maps(pkg, ny, nx, kt=kt)
    assert used == (kt if kt else 1)


def test_wall_values_equal(pkg):
    """CR == CL is allowed: nothing is divided by it."""
    ff, _, _, _ = check_maps(pkg, 9, 7, cl=0.75, cr=0.75)
    assert np.all(np.isfinite(ff.sections))


@pytest.mark.parametrize("ny,nx", [(9, 7), (16, 130)])
def test_stack_equals_one_image_contexts(pkg, ny, nx):
    """A stack of 3 against three one-image contexts given each image's field and D: the same bits, and no fy across an image's
    last row."""
    nimg = 3
    ff, x, D, used = check_maps(pkg, ny, nx, nimg=nimg)
    assert np.all(ff.fy[:, -1, :] == 0.0)
    for k in range(nimg):
        with pkg.Solver(nx, ny) as s:
            s.set_field(x[k])
            one = s.flux_field(D[k], CL, CR)
            assert s.plan_value("flux_kt") == used
        for name, a, b in zip(one._fields, one, (ff.fx[k], ff.fy[k], ff.left[k:k + 1], ff.sections[k:k + 1])):
            assert_same(a, b, (name, k))


@pytest.mark.parametrize("phases", [2, 3])
def test_image_system_form(pkg, oracle, phases):
    """deff_flux_field on assemble_2phase and on assemble_3phase without a grid: the bits of flux_field(D) with the oracle's plane."""
    ny, nx = 20, 33
    pix = np.random.default_rng(phases).integers(0, 256, (ny, nx), dtype=np.uint8)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        if phases == 2:
            s.assemble_2phase(1e-3, 1.0, CL, CR)
            D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
        else:
            s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR)
            D = oracle.fill_D_3phase(pix, 1.0, 1e-3, 10.0)
            assert len(np.unique(D)) == 3
        s.init_linear(CL, CR)
        s.sweeps(5)
        x = s.get_field()
        a = s.flux_field()
        b = s.flux_field(D, CL, CR)
        kt = s.plan_value("flux_kt")
    want = model_stack(x[None], D[None], CL, CR, kt)
    for name, u, v, w in zip(a._fields, a, b, want):
        assert np.array_equal(u, v), name
        assert_same(u, w, name)


@pytest.mark.parametrize("ny,nx", [(24, 31), (64, 130)])
def test_conservation_on_a_converged_field(pkg, ny, nx):
    """After solve_cg(rtol=1e-12) every section carries the same flux: Q[j + 1] - Q[j] = -sum over the rows of r[:, j] exactly
    (the fy terms telescope), r = A x - b, so max_j |Q[j] - Q[0]| <= ||b - A x||_1 + 8 ny 2^-53 max_j sum_rows |F_j| for the
    rounding of the sums; and (Q[0] + Q[W]) / (2 (CR - CL)) is flux()'s deff_raw within the host test's bound."""
    D = make_D(ny, nx, zeros=0.05)[0]
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)                             # a D per cell has no row dictionary
        r = s.solve_cg(rtol=1e-12)
        assert r.converged
        A, b = s.get_system()
        x = s.get_field()
        ff = s.flux_field(D, CL, CR)
        deff_raw = s.flux()[0]
    Al = A.reshape(ny, nx, 5).astype(np.longdouble)              # P, W, E, S (row + 1), N (row - 1)
    xl = np.pad(x.astype(np.longdouble), 1)
    nb = np.stack([xl[1:-1, 1:-1], xl[1:-1, :-2], xl[1:-1, 2:], xl[2:, 1:-1], xl[:-2, 1:-1]], axis=-1)
    r1 = float(np.sum(np.abs(b.reshape(ny, nx) - np.sum(Al * nb, axis=-1))))
    Q = ff.sections[0]
    F = np.concatenate([ff.left.reshape(ny, 1), ff.fx], axis=1)
    rounding = 8 * ny * U * float(np.max(np.sum(np.abs(F), axis=0)))
    spread = float(np.max(np.abs(Q - Q[0])))
    print(f"flux conservation {ny}x{nx}: spread {spread:.3e}, ||b - A x||_1 {r1:.3e}, rounding term {rounding:.3e}, Q[0] {Q[0]!r}")
    assert spread <= r1 + rounding, (spread, r1, rounding)
    got = (Q[0] + Q[nx]) / (2 * (CR - CL))
    bar = 8 * ny * U * (np.sum(np.abs(ff.left)) + np.sum(np.abs(ff.fx[:, -1]))) / (2 * abs(CR - CL))
    print(f"flux conservation {ny}x{nx}: deff from the wall sections {got!r}, flux() {deff_raw!r}, bar {bar:.3e}")
    assert abs(got - deff_raw) <= bar, (got, deff_raw, bar)


def test_nothing_else_moves(pkg, oracle):
    """After flux_field the field, get_system, the sensitivity map and a following solve_cg are those of a context that never
    called it."""
    ny, nx = 40, 67                                               # odd width: a pad column
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    Dp = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    out = []
    for call in (False, True):
        with pkg.Solver(nx, ny) as s:
            s.set_image(pix)
            s.assemble_2phase(1e-3, 1.0, CL, CR)
            s.init_linear(CL, CR)
            s.sweeps(5)
            s.sensitivity()
            p0, pitch = s.device_sensitivity_ptr()
            if call:
                ff, ms = s.flux_field(timing=True)[:4], s.flux_field(Dp, CL, CR, timing=True)[4]
                assert ms > 0.0 and np.all(np.isfinite(ff[3]))
                assert s.device_sensitivity_ptr() == (p0, pitch)
            x = s.get_field()
            A, b = s.get_system()
            smap = device_rows(p0, ny, pitch)
            r = s.solve_cg(rtol=1e-10)
            out.append((x, A, b, smap, s.get_field(), (r.iters, r.rel_residual, r.deff_raw, r.converged)))
    for u, v in zip(out[0][:5], out[1][:5]):
        assert np.array_equal(u, v)
    assert out[0][5] == out[1][5], (out[0][5], out[1][5])


def test_refusals(pkg, oracle):
    ny, nx = 20, 33
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    D = make_D(ny, nx)[0]
    with pkg.Solver(nx, ny) as s:
        _refused(pkg, s.device_flux_field_ptrs, -5)              # DEFF_ESTATE before the first call
        _refused(pkg, lambda: s.flux_field(D, CL, CR), -5, "no field")
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        _refused(pkg, s.flux_field, -5, "no field")
        _refused(pkg, s.device_flux_field_ptrs, -5)
        x = swept(s, D[None])[0]                                 # (assemble_from_D: no image system any more)
        _refused(pkg, s.flux_field, -5, "assembled from the image")
        ff = s.flux_field(D, CL, CR)
        px, py, pitch = s.device_flux_field_ptrs()
        dev = device_rows(px, ny, pitch), device_rows(py, ny, pitch)
        assert np.array_equal(dev[0][:, :nx], ff.fx) and np.array_equal(dev[1][:, :nx], ff.fy)

        def unchanged():
            assert s.device_flux_field_ptrs() == (px, py, pitch)
            assert np.array_equal(device_rows(px, ny, pitch), dev[0]) and np.array_equal(device_rows(py, ny, pitch), dev[1])

        L = pkg._capi.load()
        assert L.deff_flux_field_D(s._ctx, None, CL, CR, None, None, None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        unchanged()
        s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR, grid=np.zeros((ny, nx), dtype=np.uint32))
        s.set_field(x)
        _refused(pkg, s.flux_field, -1, "Grid")
        unchanged()
        s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR)
        s.set_field(x)
        _refused(pkg, s.flux_field, -1, "Grid")
        unchanged()
        s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR)               # ... and without a Grid the same context goes through
        s.set_field(x)
        got = s.flux_field()
        want = fm.flux_field(x, oracle.fill_D_3phase(pix, 1.0, 1e-3, 10.0), CL, CR)
        assert np.array_equal(got.fx, want[0]) and np.array_equal(got.fy, want[1]) and np.array_equal(got.left[0], want[2])
        # every output may be NULL
        Dc = np.ascontiguousarray(D)
        import ctypes as C
        assert L.deff_flux_field_D(s._ctx, Dc.ctypes.data_as(C.c_void_p), CL, CR, None, None, None, None, None) == 0
        assert np.array_equal(device_rows(s.device_flux_field_ptrs()[0], ny, pitch), dev[0])


def test_flux_vectors(pkg):
    """The package's cell-centred flux densities of a GPU flux field against the model's."""
    ny, nx = 9, 7
    ff, _, _, _ = check_maps(pkg, ny, nx)
    Jx, Jy = pkg.flux_vectors(ff, nx, ny)
    wx, wy = fm.flux_vectors(ff.fx, ff.fy, ff.left[0])
    assert Jx.shape == Jy.shape == (ny, nx)
    assert np.array_equal(Jx, wx) and np.array_equal(Jy, wy)
    assert np.sum(Jx) < 0.0                                      # CR > CL: the concentration rises with x, the physical flux runs against it
