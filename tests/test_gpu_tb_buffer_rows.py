"""The streaming kernel's rows through buffer descriptors (tb_strip, kernels_tb.hpp): lanes outside the mesh or outside a strip's
own columns carry an out-of-range lane offset, rows outside a chunk's window take a zero-length descriptor, and the hardware's
range check does what selects, clamped addresses and branches around the stores did before.  The results are bit-identical by
construction; these are the smallest shapes at which a mask or an offset can be wrong, each against the CPU oracle with
array_equal: strips with two owned columns or nearly none, chunks shorter than, equal to and longer than the halo, every
placement of the first strip, a remainder after a blocked pass, omega = 1, the contracted arithmetic, the guarded system, a stack
with a frozen image, row slabs, dealt tiles.

Shapes are (nx, ny).  A context of fewer than 8 rows per image does not take the blocked kernel at all (resolve_kernel): the
2 x 3 image and the stack of 130 x 7 images run on the single-sweep kernel, which is why (2, 11) and a stack of 130 x 9 images
stand beside them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OMEGAS = (2.0 / 3.0, 1.0)


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def rand_mask(rng, nx, ny, p=0.5):
    return np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("T", [8, 6, 4])
@pytest.mark.parametrize("shape", [(2, 3), (2, 11), (112, 17), (114, 17), (128, 9), (130, 50), (226, 21)])
def test_single_image(pkg, oracle, shape, T):
    """tb_LY 1 / 5 / 16 x tb_wall_halo 0 / 1 / 2 x sweep counts T and 2 T + 1 x omega 2/3 and 1."""
    nx, ny = shape
    rng = np.random.default_rng(nx * 11 + ny * 5 + T)
    pix = rand_mask(rng, nx, ny, 0.55)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    x0 = rng.random((ny, nx))
    want = {(n, w): oracle.sweeps(A, b, x0, n, omega=w) for n in (T, 2 * T + 1) for w in OMEGAS}
    for LY in (1, 5, 16):
        for wall_halo in (0, 1, 2):
            with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
                s.set_tuning("tb_impl", 1)
                s.set_tuning("tb_T", T)
                s.set_tuning("tb_LY", LY)
                s.set_tuning("tb_wall_halo", wall_halo)
                s.set_image(pix)
                s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                for (n, w), ref in want.items():
                    s.set_field(x0)
                    s.sweeps(n, w)
                    if ny >= 8:
                        launches, per = s.last_launches()
                        assert s.kernel_in_use() == "matfree_tb" and s.plan()["tb_impl"] == 1
                        assert per == T and launches == n // T + n % T
                    assert np.array_equal(s.get_field(), ref), (LY, wall_halo, n, w)


@pytest.mark.parametrize("T", [8, 4])
def test_contracted_arithmetic(pkg, oracle, T):
    nx, ny = 130, 50
    rng = np.random.default_rng(31 + T)
    pix = rand_mask(rng, nx, ny, 0.45)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-2)
    A, b = oracle.discretize(D, 0.1, 0.93)
    x0 = rng.random((ny, nx))
    n = 2 * T + 1
    want = oracle.sweeps(A, b, x0, n, flavour="fma")
    assert not np.array_equal(want, oracle.sweeps(A, b, x0, n))
    with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
        for k, v in (("tb_impl", 1), ("tb_T", T), ("tb_LY", 5), ("fma", 1)):
            s.set_tuning(k, v)
        s.set_image(pix)
        s.assemble_2phase(1e-2, 1.0, 0.1, 0.93)
        s.set_field(x0)
        s.sweeps(n)
        assert s.kernel_in_use() == "matfree_tb" and s.plan()["tb_impl"] == 1
        assert np.array_equal(s.get_field(), want)


@pytest.mark.parametrize("T", [8, 4])
def test_guarded_three_phase_zero_diffusivity(pkg, oracle, T):
    """Solid of zero diffusivity: links are -0.0, the guarded kernel (GUARD) keeps the reference's non-zero test on every link."""
    nx, ny = 114, 17
    rng = np.random.default_rng(22 + T)
    pix = rng.choice(np.array([0, 120, 255], dtype=np.uint8), size=(ny, nx), p=[0.3, 0.4, 0.3])
    D = oracle.fill_D_3phase(pix, 1.0, 0.0, 50.0)
    grid = (pix > 200).astype(np.uint32)
    with np.errstate(all="ignore"):
        A, b = oracle.discretize(D, 0.0, 1.0, grid=grid)
        x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
        want = oracle.sweeps(A, b, x0, 2 * T + 1)
    for LY in (1, 5, 16):
        with pkg.Solver(nx, ny) as s:
            for k, v in (("tb_impl", 1), ("tb_T", T), ("tb_LY", LY), ("tb_wall_halo", LY % 3)):
                s.set_tuning(k, v)
            s.set_image(pix)
            s.assemble_3phase(0.0, 1.0, 50.0, 0.0, 1.0, grid=grid)
            s.init_linear(0.0, 1.0)
            s.sweeps(2 * T + 1)
            assert s.kernel_in_use() == "matfree_tb" and s.plan()["tb_impl"] == 1
            assert np.array_equal(s.get_field(), want, equal_nan=True), LY


@pytest.mark.parametrize("T", [8, 4])
@pytest.mark.parametrize("ny", [7, 9])
def test_stack_with_the_middle_image_frozen(pkg, oracle, ny, T):
    """3 images of 130 x ny, chunks of 4 rows.  The middle image is all fluid and starts from its solution, the linear ramp: it
    stops at the first check and stays frozen while its neighbours sweep on.  Every image must be its own single-image run -- a
    store that reached a neighbouring image, or touched the frozen one, would show."""
    nx, B = 130, 3
    rng = np.random.default_rng(5 + ny)
    pixs = [rand_mask(rng, nx, ny, 0.5), np.zeros((ny, nx), np.uint8), rand_mask(rng, nx, ny, 0.6)]
    with pkg.Solver(nx, ny, nimg=B, kernel="matfree_tb") as s:
        for k, v in (("tb_impl", 1), ("tb_T", T), ("tb_LY", 4)):
            s.set_tuning(k, v)
        s.set_image(np.stack(pixs))
        s.assemble_2phase(1e-2, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        res = s.solve(1e-3, 3000, check_every=100)
        got = s.get_field()
        if ny >= 8:
            assert s.kernel_in_use() == "matfree_tb" and s.plan()["tb_impl"] == 1
    iters = []
    for k in range(B):
        D = oracle.fill_D_2phase(pixs[k], 1.0, 1e-2)
        A, b = oracle.discretize(D, 0.0, 1.0)
        it, deff, conv, x, _, _ = oracle.jacobi(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), D, 0.0, 1.0, 1e-3, 3000, check_every=100)
        assert (res[k].iters, res[k].deff_raw, res[k].conv) == (it, deff, conv), k
        assert np.array_equal(got[k * ny:(k + 1) * ny], x), k
        iters.append(it)
    assert iters[1] < min(iters[0], iters[2]), iters             # the middle image was frozen while the others went on


@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("T", [8, 4])
@pytest.mark.parametrize("nx,NY,nslabs", [(130, 40, 2), (114, 33, 3)])
def test_row_slabs(pkg, oracle, nx, NY, nslabs, T, overlap):
    """Owned-row and halo masks ride on the same descriptors: the slabs' field is the oracle's and the single context's."""
    rng = np.random.default_rng(nx + NY + T)
    pix = rand_mask(rng, nx, NY, 0.55)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    x0 = rng.random((NY, nx))
    n = 3 * T + 2
    want = oracle.sweeps(A, b, x0, n)
    with pkg.Solver(nx, NY, kernel="matfree_tb") as s:
        s.set_tuning("tb_impl", 1)
        s.set_tuning("tb_T", T)
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.set_field(x0)
        s.sweeps(n)
        single = s.get_field()
    assert np.array_equal(single, want)
    with pkg.SlabGroup(nx, NY, [0] * nslabs) as g:
        g.set_tuning("slab_overlap", overlap)
        g.set_tuning("tb_impl", 1)
        g.set_tuning("tb_T", T)
        g.set_image(pix)
        g.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        g.set_field(x0)
        g.sweeps(n)
        assert all(p["tb_impl"] == 1 and p["tb_T"] == T for p in g.plans())
        assert np.array_equal(g.get_field(), single)


@pytest.mark.parametrize("shape", [(130, 50), (226, 31)])
def test_dealt_tiles_at_a_small_shape(pkg, oracle, shape):
    """With no tb_LY given, passes of eight sweeps and at least 24 rows the planner deals the chunks by wave rank (the `dealt`
    table of the kernel) at any size: the other way into tb_strip."""
    nx, ny = shape
    rng = np.random.default_rng(nx + ny)
    pix = rand_mask(rng, nx, ny, 0.5)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    A, b = oracle.discretize(D, 0.0, 1.0)
    x0 = rng.random((ny, nx))
    for wall_halo in (0, 1, 2):
        with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
            for k, v in (("tb_impl", 1), ("tb_T", 8), ("tb_wall_halo", wall_halo)):
                s.set_tuning(k, v)
            s.set_image(pix)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            for w in OMEGAS:
                s.set_field(x0)
                s.sweeps(17, w)
                assert s.plan()["tb_impl"] == 1 and s.plan()["tb_ranked"] == 1, s.plan()
                assert np.array_equal(s.get_field(), oracle.sweeps(A, b, x0, 17, omega=w)), (wall_halo, w)
