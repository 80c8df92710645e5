"""tests/dict_cases.py on the CPU: the host model of the row dictionary harvest orders rows by its written rule, and the
builder reaches the exact row count of every (shape, K, kind) that tests/test_gpu_dict.py runs."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as dc


def test_library_declares_the_dictionary_readback():
    from effectivediffusivityfvm_amd import _capi
    from effectivediffusivityfvm_amd.solver import Solver
    assert "deff_get_dictionary" in _capi.SYMBOLS and hasattr(_capi.load(), "deff_get_dictionary")
    assert callable(Solver.dictionary)


def test_model_orders_rows_by_population_then_bits():
    """A hand-made system of width 4: populations 3, 2, 2, 1 -- the two rows of population 2 differ in the sign of b only and
    -0.0 (bit 63 set) sorts after +0.0 as an unsigned integer; a negative aW sorts after every positive one."""
    r_big = [4.0, -1.0, -1.0, -1.0, -1.0, 0.0]
    r_pos = [2.0, 0.5, 0.0, 0.0, 0.0, 0.0]
    r_neg = [2.0, 0.5, 0.0, 0.0, 0.0, -0.0]
    r_one = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    cells = [r_neg, r_big, r_pos, r_big, r_one, r_neg, r_pos, r_big]
    R = np.array(cells)
    m = dc.count_rows(R[:, :5], R[:, 5], 4)
    assert m.count == 4 and m.table.shape == (5, 6)
    want = np.array([[0.0] * 6, r_big, r_pos, r_neg, r_one])
    assert np.array_equal(dc.bit_view(m.table), dc.bit_view(want))
    assert np.array_equal(m.codes, np.array([[24, 8, 16, 8], [32, 24, 16, 8]], dtype=np.uint16))
    # the order is the one of a plain Python sort on (-population, the six integers)
    keys = sorted({tuple(dc.bit_view(np.array(c)).tolist()) for c in cells},
                  key=lambda t: (-sum(tuple(dc.bit_view(np.array(c)).tolist()) == t for c in cells), t))
    assert [tuple(dc.bit_view(row).tolist()) for row in m.table[1:]] == keys


def test_model_seats_the_pad_row_of_an_odd_width():
    """Width 3: the pad column's identity row is one more row with population = mesh rows, unless the mesh has it already."""
    r = [4.0, -1.0, -1.0, -1.0, -1.0, 0.25]
    R = np.array([r] * 6)
    m = dc.count_rows(R[:, :5], R[:, 5], 3)
    assert m.count == 2 and m.codes.shape == (2, 4)
    assert np.array_equal(m.codes, np.array([[8, 8, 8, 16]] * 2, dtype=np.uint16))
    assert np.array_equal(m.table[2], dc.IDENTITY)
    R[4] = dc.IDENTITY                                   # a mesh cell with the identity row: population 3 against 5
    m = dc.count_rows(R[:, :5], R[:, 5], 3)
    assert m.count == 2
    assert np.array_equal(m.codes, np.array([[8, 8, 8, 16], [8, 16, 8, 16]], dtype=np.uint16))
    # an even width has no pad row
    assert dc.count_rows(R[:, :5], R[:, 5], 2).codes.shape == (3, 2)


def test_bases_have_the_expected_rows(oracle):
    """Half-and-half masks: 92 ... 97 distinct rows and no identity row, at every shape of the GPU tests and at 160 x 128."""
    for nx, ny in ((64, 40), (65, 41), (130, 71), (160, 128)):
        A, b, _, _ = dc.base_system(oracle, nx, ny, 1, dc.seed_of(nx, ny, 1, None, "b"))
        R = dc.bit_view(np.column_stack([A, b]))
        n = len(np.unique(R, axis=0))
        assert 85 <= n <= 110, (nx, ny, n)
        assert not (R == dc.bit_view(dc.IDENTITY)).all(axis=1).any()
        assert dc.count_rows(A, b, nx).count == n + (nx & 1)


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("K", dc.KS + [512])
@pytest.mark.parametrize("nx,ny,nimg", dc.SHAPES)
def test_builder_reaches_the_exact_count(oracle, nx, ny, nimg, K, kind):
    s = dc.case(oracle, nx, ny, nimg, K, kind)
    m = dc.count_rows(s.A, s.b, nx)
    assert m.count == s.K and (K is None or s.K == K)
    assert m.table.shape == (s.K + 1, 6) and m.codes.shape == (nimg * ny, nx + (nx & 1))
    # the expansion of the model's own codes is the system, bit for bit
    back = m.table[m.codes[:, :nx].astype(np.int64) >> 3].reshape(-1, 6)
    assert np.array_equal(dc.bit_view(back), dc.bit_view(np.column_stack([s.A, s.b])))
    col = np.arange(s.b.size) % nx
    inner = (col > 0) & (col < nx - 1)
    A0, b0, _, _ = dc.base_system(oracle, nx, ny, nimg, dc.seed_of(nx, ny, nimg, K, kind),
                                  dc.sparse_p(nx, ny) if K is not None and K < 90 else 0.5)
    if kind == "b":
        assert np.array_equal(s.A, A0)
        assert (s.b[inner] != 0).any() == (K is not None)            # sources inside the domain: b is looked up everywhere
    else:
        assert np.array_equal(s.b, b0) and np.all(s.b[inner] == 0)   # the right-hand side stays on the walls
        assert np.array_equal(s.A[:, 1:], A0[:, 1:])                 # links untouched: still symmetric
        # a larger diagonal only: as dominant as the base (whose diagonal is the links' sum up to its own rounding)
        assert np.all(s.A[:, 0] >= A0[:, 0]) and np.all(s.A[:, 0] >= -s.A[:, 1:].sum(axis=1) * (1 - 2.0 ** -50))
    if nx & 1:
        pad = m.codes[:, nx]
        assert (pad == pad[0]).all() and np.array_equal(m.table[pad[0] >> 3], dc.IDENTITY)


def test_systems_of_the_limits(oracle):
    """2 560 rows at 64 x 40 and 20 480 at 160 x 128 (more than the hash table's slots) from a uniform-random D."""
    s = dc.uniform_D_system(oracle, 64, 40, 21)
    assert dc.count_rows(s.A, s.b, 64).count == 2560 > dc.LUT_MAX_ROWS - 1
    s = dc.uniform_D_system(oracle, 160, 128, 22)
    assert dc.count_rows(s.A, s.b, 160).count == 20480 > dc.DICT_SLOTS


def test_pair_with_and_without_a_source_inside(oracle):
    clear, source, cell = dc.allb_pair(oracle)
    assert dc.count_rows(clear.A, clear.b, 260).count == dc.count_rows(source.A, source.b, 260).count == 511
    col = np.arange(clear.b.size) % 260
    inner = (col > 0) & (col < 259)
    assert np.all(clear.b[inner] == 0) and np.flatnonzero(source.b[inner] != 0).tolist() == [np.flatnonzero(inner).tolist().index(cell)]
    assert 128 <= cell % 260 <= 131 and np.array_equal(clear.A, source.A)


def test_near_equal_rows(oracle):
    s, changes = dc.near_equal_system(oracle)
    m = dc.count_rows(s.A, s.b, s.nx)
    assert m.count == s.K == 43
    R = dc.bit_view(np.column_stack([s.A, s.b]))
    for cell, plane in changes:
        # some other cell's row equals this cell's in the five other planes and is its neighbour in this one: one unit in the
        # last place apart, or the same zero with the other sign
        rest = [k for k in range(6) if k != plane]
        twins = R[(R[:, rest] == R[cell, rest]).all(axis=1) & (R[:, plane] != R[cell, plane]), plane]
        gaps = {abs(int(t) - int(R[cell, plane])) for t in twins}
        assert (1 << 63 if plane == 5 else 1) in gaps, (cell, plane, sorted(gaps)[:4])
    cell, plane = changes[2]
    assert R[cell, 5] == 1 << 63 and cell % s.nx == 0                # -0.0 in the first column
