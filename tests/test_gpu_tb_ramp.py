"""The straight-line ramp of tb_strip (kernels_tb.hpp): a tile whose window starts a full halo above its chunk runs its first
18 steps (T = 8) as straight code with exactly the levels each step needs, twelve rows requested ahead; tiles at the top of a
mesh keep the generic trimmed groups.  Which rows are swept, by whom and in which arithmetic is unchanged, so the fields are
those of the oracle and of "tb_chain" 0 bit for bit -- on the smallest shapes at which the ramp can go wrong, each asserted
from the plan ("tb_chunk_min" / "tb_chunk_max": rows of the shortest and of the tallest dealt chunk):

  one strip, chunks of about T rows       the ramp is three quarters of every tile
  a last chunk of 1 row, and one of 2     fewer output rows than the ramp has steps
  1030 x 4000                             chunks of 20 / 12 / 8 rows: several rounds of the steady-state loop behind the ramp
  a stack of 3 images                     tiles at the top of a mesh in the middle of the array keep the generic groups
  two row slabs through SlabGroup         the mesh begins above the array (dom_lo < 0); slab plans are not dealt and not
                                          chained, so their tiles keep the generic groups -- the fields must not notice
  tb_wall_halo = 1 on 226 columns         the wall column in a strip's halo

after 2 T, 3 T and 5 T + 3 sweeps, omega 2/3 and 1.  Every run of a Solver asserts that the plan WAS chained (or was not, for
"tb_chain" 0) and that nothing fell back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 8
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


def run(pkg, pix, x0, n, chain, omega=2.0 / 3.0, tune=None, nimg=1, chunks=None):
    """The field after n sweeps of one sweeps() call; chunks = (shortest, tallest) dealt chunk the plan must report, or a
    predicate on the two."""
    ny, nx = pix.shape[0] // nimg, pix.shape[1]
    with pkg.Solver(nx, ny, nimg=nimg, kernel="matfree_tb") as s:
        for k, v in dict(BASE, **(tune or {}), tb_chain=chain).items():
            s.set_tuning(k, v)
        s.set_image(pix if nimg == 1 else pix.reshape(nimg, ny, nx))
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.set_field(x0)
        s.sweeps(n, omega)
        check_plan(s, chain)
        got = (s.plan_value("tb_chunk_min"), s.plan_value("tb_chunk_max"))
        if chunks is not None:
            assert chunks(*got) if callable(chunks) else got == chunks, got
        return s.get_field()


def both_against_the_oracle(pkg, oracle, pix, x0, counts=COUNTS, omegas=OMEGAS, **kw):
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    for om, kern in omegas:
        for n in counts:
            want = oracle.sweeps(A, b, x0, n, kernel=kern, omega=om)
            got = run(pkg, pix, x0, n, 1, om, **kw)
            flat = run(pkg, pix, x0, n, 0, om, **kw)
            assert np.array_equal(got, flat), (om, n)
            assert np.array_equal(got, want), (om, n)


# (97 columns: one strip.  The heights: 241 rows are cut into 30 chunks of 7 ... 9 rows; 243 and 244 rows leave the youngest
# rank's last chunk one row and two rows)
REMAINDER_1, REMAINDER_2 = 243, 244


@pytest.mark.parametrize("ny,chunks", [(241, lambda lo, hi: lo >= 1 and hi <= T + 1),
                                       (REMAINDER_1, lambda lo, hi: lo == 1), (REMAINDER_2, lambda lo, hi: lo == 2)])
def test_one_strip_of_short_chunks(pkg, oracle, ny, chunks):
    nx = 97
    rng = np.random.default_rng(nx * 11 + ny)
    both_against_the_oracle(pkg, oracle, rand_mask(rng, nx, ny), rng.random((ny, nx)), chunks=chunks)


def test_tall_chunks_run_the_steady_loop_behind_the_ramp(pkg, oracle):
    nx, ny = 1030, 4000
    rng = np.random.default_rng(4000)
    both_against_the_oracle(pkg, oracle, rand_mask(rng, nx, ny), rng.random((ny, nx)), counts=(2 * T, 5 * T + 3), omegas=OMEGAS[:1],
                            chunks=lambda lo, hi: lo <= 8 and hi >= 20)
    both_against_the_oracle(pkg, oracle, rand_mask(rng, nx, ny), rng.random((ny, nx)), counts=(3 * T,), omegas=OMEGAS[1:])


def test_stack_tiles_at_the_top_of_an_image_keep_the_generic_groups(pkg, oracle):
    nx, ny, B = 130, 50, 3
    rng = np.random.default_rng(50)
    pixs = [rand_mask(rng, nx, ny, 0.4 + 0.1 * k) for k in range(B)]
    x0 = rng.random((B * ny, nx))
    for om, kern in OMEGAS:
        for n in COUNTS:
            got = run(pkg, np.concatenate(pixs), x0, n, 1, om, nimg=B)
            flat = run(pkg, np.concatenate(pixs), x0, n, 0, om, nimg=B)
            assert np.array_equal(got, flat), (om, n)
            for k in range(B):
                A, b = oracle.discretize(oracle.fill_D_2phase(pixs[k], 1.0, 1e-3), 0.0, 1.0)
                assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(A, b, x0[k * ny:(k + 1) * ny], n, kernel=kern, omega=om)), (om, n, k)


def test_wall_column_in_a_strips_halo(pkg, oracle):
    nx, ny = 226, 62
    rng = np.random.default_rng(226)
    both_against_the_oracle(pkg, oracle, rand_mask(rng, nx, ny), rng.random((ny, nx)), tune={"tb_wall_halo": 1})


def test_two_row_slabs(pkg, oracle):
    nx, NY = 226, 62
    rng = np.random.default_rng(62)
    pix, x0 = rand_mask(rng, nx, NY), rng.random((NY, nx))
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)
    for om, kern in OMEGAS:
        for n in COUNTS:
            with pkg.SlabGroup(nx, NY, [0, 0]) as g:
                for k, v in BASE.items():
                    g.set_tuning(k, v)
                g.set_image(pix)
                g.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                g.set_field(x0)
                g.sweeps(n, om)
                for k in range(2):
                    assert (g.plan_value(k, "tb_impl"), g.plan_value(k, "tb_T"), g.plan_value(k, "tb_fallbacks")) == (1, T, 0), (om, n, k)
                assert np.array_equal(g.get_field(), oracle.sweeps(A, b, x0, n, kernel=kern, omega=om)), (om, n)
