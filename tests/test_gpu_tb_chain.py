"""Chained passes of the streaming kernel (k_sweep_matfree_tb_chain): several passes of the dealt tiles in one launch, every
tile waiting only for the tiles whose rows it reads or overwrites (csrc/tb_chain.hpp).  The same tiles and the same arithmetic
as one launch per pass, so the fields are those of "tb_chain" 0 and of the oracle bit for bit -- on the smallest shapes at
which a neighbour list or a buffer swap can be wrong: one strip with many chunks, two strips, three strips whose wall strips
are cut differently from the middle one, ten strips; two passes (one swap), an odd number of passes, five passes followed by
single sweeps.  Every chained run also asserts that the plan WAS chained and that no launch fell back: a silent fallback
would compute the same bits without running the new kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 8
SHAPES = [(97, 241), (130, 50), (226, 31), (300, 200), (1030, 137)]
COUNTS = (2 * T, 3 * T, 5 * T + 3)
OMEGAS = ((2.0 / 3.0, 0), (1.0, 1))                      # (omega, the oracle's kernel: updateX_SOR, updateX_V1)
BASE = {"tb_impl": 1, "tb_T": T}


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def rand_mask(rng, nx, ny, p=0.5):
    return np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8)


def check_plan(s, chain):
    assert s.kernel_in_use() == "matfree_tb"
    p = s.plan()
    assert (p["tb_impl"], p["tb_T"], p["tb_ranked"], p["tb_resident"]) == (1, T, 1, 0), p
    assert s.plan_value("tb_chain") == chain and s.plan_value("tb_fallbacks") == 0, (s.plan_value("tb_chain"), s.plan_value("tb_fallbacks"))


def run(pkg, pix, x0, counts, chain, omega=2.0 / 3.0, tune=None, nimg=1):
    """The fields after counts[0], counts[0] + counts[1], ... sweeps, each count one sweeps() call."""
    ny, nx = pix.shape[0] // nimg, pix.shape[1]
    out = []
    with pkg.Solver(nx, ny, nimg=nimg, kernel="matfree_tb") as s:
        for k, v in dict(BASE, **(tune or {}), tb_chain=chain).items():
            s.set_tuning(k, v)
        s.set_image(pix if nimg == 1 else pix.reshape(nimg, ny, nx))
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.set_field(x0)
        for n in counts:
            s.sweeps(n, omega)
            launches, per = s.last_launches()
            assert (launches, per) == (n // T + n % T, T)                  # a chained launch counts its passes
            check_plan(s, chain)
            out.append(s.get_field())
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """Per shape: image, start field, and the oracle's field after every count of COUNTS, for both omegas (computed once)."""
    out = {}
    for nx, ny in SHAPES:
        rng = np.random.default_rng(nx * 11 + ny)
        pix = rand_mask(rng, nx, ny)
        A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
        x0 = rng.random((ny, nx))
        want = {(om, n): oracle.sweeps(A, b, x0, n, kernel=kern, omega=om) for om, kern in OMEGAS for n in COUNTS}
        out[(nx, ny)] = (pix, x0, want)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_chained_vs_unchained_and_oracle(pkg, cases, shape):
    pix, x0, want = cases[shape]
    for om, _ in OMEGAS:
        for n in COUNTS:
            got, = run(pkg, pix, x0, [n], 1, om)
            flat, = run(pkg, pix, x0, [n], 0, om)
            assert np.array_equal(got, flat), (om, n)
            assert np.array_equal(got, want[(om, n)]), (om, n)


SKEWS = ({"tb_rank_w0": 900, "tb_rank_w1": 60, "tb_rank_w2": 40}, {"tb_rank_wall": 2500},
         {"tb_rank_w0": 700, "tb_rank_w1": 200, "tb_rank_w2": 100, "tb_rank_wall": 2500})


@pytest.mark.parametrize("shape", [(300, 200), (1030, 137)])
def test_chained_with_skewed_tables(pkg, cases, shape):
    """Skewed rank speeds and a heavy wall surcharge: the wall strips' chunk boundaries fall differently from the inner strips'
    (rows per rank, wall / inner, with the surcharge: 8 9 8 / 9 8 8 at 300 x 200, 10 10 8 / 12 8 8 / 11 9 8 at 1030 x 137)."""
    pix, x0, want = cases[shape]
    n = 5 * T + 3
    for tune in SKEWS:
        got, = run(pkg, pix, x0, [n], 1, tune=tune)
        assert np.array_equal(got, want[(2.0 / 3.0, n)]), tune


def test_chained_with_skewed_tables_of_tall_chunks(pkg, oracle):
    """Chunks of these shapes are about T rows whatever the weights (every wave of the chip gets one).  The weights only tell
    once strips x rows exceed the chip's 3 072 waves by far: ten strips of 4 000 rows are cut into 102-103 chunks per rank of
    20 / 12 / 8 rows (22 / 8 / 8, 9 / 14 / 17, and 15 / 13 / 10 in the wall strips beside 20 / 12 / 8, with the tables below),
    so a tile's window meets up to six chunks of the next strip."""
    nx, ny = 1030, 4000
    rng = np.random.default_rng(4000)
    pix = rand_mask(rng, nx, ny)
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    x0 = rng.random((ny, nx))
    n = 2 * T + 3
    want = oracle.sweeps(A, b, x0, n)
    for tune in SKEWS + ({}, {"tb_rank_w0": 250, "tb_rank_w1": 350, "tb_rank_w2": 400}):
        got, = run(pkg, pix, x0, [n], 1, tune=tune)
        assert np.array_equal(got, want), tune


def test_chained_contracted_arithmetic(pkg, oracle, cases):
    pix, _, _ = cases[(300, 200)]
    ny, nx = pix.shape
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0, flavour="fma")
    n = 3 * T
    want = oracle.sweeps(A, b, x0, n, flavour="fma")
    got, = run(pkg, pix, x0, [n], 1, tune={"fma": 1})
    assert np.array_equal(got, want)


def test_chained_dictionary_system(pkg, oracle):
    """Rows harvested from a caller's matrix (three permeable classes) through set_system."""
    nx, ny = 300, 200
    rng = np.random.default_rng(6)
    pix = np.where(rng.random((ny, nx)) < 0.3, 255, np.where(rng.random((ny, nx)) < 0.5, 120, 0)).astype(np.uint8)
    pix[0] = pix[-1] = 255
    D = oracle.fill_D_3phase(pix, 1.0, 0.5, 30.0)
    A, b = oracle.discretize(D, 0.0, 1.0)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    n = 5 * T + 3
    want = oracle.sweeps(A, b, x0, n)
    for chain in (1, 0):
        with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
            for k, v in dict(BASE, tb_chain=chain).items():
                s.set_tuning(k, v)
            s.set_system(A, b, D, 0.0, 1.0)
            s.set_field(x0)
            s.sweeps(n)
            check_plan(s, chain)
            assert np.array_equal(s.get_field(), want)


def test_chained_stack_neighbours_stay_inside_an_image(pkg, oracle):
    nx, ny, B = 130, 40, 3
    rng = np.random.default_rng(40)
    pixs = [rand_mask(rng, nx, ny, 0.4 + 0.1 * k) for k in range(B)]
    x0 = rng.random((B * ny, nx))
    n = 5 * T + 3
    got, = run(pkg, np.concatenate(pixs), x0, [n], 1, nimg=B)
    for k in range(B):
        A, b = oracle.discretize(oracle.fill_D_2phase(pixs[k], 1.0, 1e-3), 0.0, 1.0)
        assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(A, b, x0[k * ny:(k + 1) * ny], n)), k


def test_two_chained_calls_in_a_row(pkg, cases):
    """The flags count passes since they were cleared: the second call starts where the first one's count ended."""
    pix, x0, want = cases[(300, 200)]
    a, b = run(pkg, pix, x0, [2 * T, T], 1)                                   # 2T, then T more (one pass: not chained, same table)
    assert np.array_equal(a, want[(2.0 / 3.0, 2 * T)]) and np.array_equal(b, want[(2.0 / 3.0, 3 * T)])
    a, b = run(pkg, pix, x0, [3 * T, 2 * T + 3], 1)
    assert np.array_equal(a, want[(2.0 / 3.0, 3 * T)]) and np.array_equal(b, want[(2.0 / 3.0, 5 * T + 3)])


def test_chained_solve_equals_unchained(pkg, cases):
    pix, _, _ = cases[(300, 200)]
    ny, nx = pix.shape
    res = {}
    for chain in (1, 0):
        with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
            for k, v in dict(BASE, tb_chain=chain).items():
                s.set_tuning(k, v)
            s.set_image(pix)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            r = s.solve(1e-4, 2000, check_every=40)
            check_plan(s, chain)
            res[chain] = (r.iters, r.deff_raw, r.conv, s.get_field())
    assert res[1][0] >= 80 and res[1][:3] == res[0][:3]
    assert np.array_equal(res[1][3], res[0][3])


def test_two_chained_contexts_on_one_device(pkg, cases):
    """Two contexts called alternately: each has its own flags and count; their launches never share the chip."""
    pa, xa, wa = cases[(300, 200)]
    pb, xb, wb = cases[(130, 50)]
    with pkg.Solver(300, 200, kernel="matfree_tb") as s1, pkg.Solver(130, 50, kernel="matfree_tb") as s2:
        for s, pix, x0 in ((s1, pa, xa), (s2, pb, xb)):
            for k, v in dict(BASE, tb_chain=1).items():
                s.set_tuning(k, v)
            s.set_image(pix)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.set_field(x0)
        s1.sweeps(2 * T); s2.sweeps(3 * T); s1.sweeps(T); s2.sweeps(2 * T + 3)
        check_plan(s1, 1); check_plan(s2, 1)
        assert np.array_equal(s1.get_field(), wa[(2.0 / 3.0, 3 * T)])
        assert np.array_equal(s2.get_field(), wb[(2.0 / 3.0, 5 * T + 3)])
