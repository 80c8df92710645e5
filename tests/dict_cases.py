"""Host model of the row dictionary harvest (csrc/kernels_dict.hpp, csrc/api_dict.hip) and systems built to an exact number of
distinct rows (test infrastructure only; tests/test_dict_cases_host.py and tests/test_gpu_dict.py).

The model restates the rule of DESIGN.md ("Row dictionary: code order"): the distinct rows of [A | b], compared on their bit
patterns, ordered by population (most cells first) and, among rows of equal population, by the six doubles' bit patterns as
unsigned 64-bit integers in plane order a0, aW, aE, aS, aN, b.  Row k of that order has code 8 (k + 1); code 0 is the zero row,
which no cell of a harvested system carries.  An odd mesh width is padded by one column of identity rows (1, 0, 0, 0, 0, 0),
which take a seat of the table like any other row."""
from collections import Counter, namedtuple

import numpy as np

LUT_MAX_ROWS = 512                      # seats of the table, the zero row included (csrc/lut_layout.hpp)
DICT_SLOTS = 1 << 14                    # slots of the harvest's hash table (csrc/kernels_dict.hpp)
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0])

Model = namedtuple("Model", "count table codes")


def bit_view(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def padded_rows(A, b, nx):
    """[A | b] as (rows, pitch, 6) with pitch = nx rounded up to even: what the harvest reads, the pad column's identity rows
    included."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, nx, 5)
    R = np.concatenate([A, np.asarray(b, dtype=np.float64).reshape(-1, nx, 1)], axis=2)
    if nx & 1:
        R = np.concatenate([R, np.broadcast_to(IDENTITY, (R.shape[0], 1, 6))], axis=1)
    return np.ascontiguousarray(R)


def count_rows(A, b, nx):
    """Model(count, table, codes) of the system A (n, 5), b (n) of width nx (a stack: image after image).  count: distinct
    rows on the bit view, plus one for an odd width's pad row unless a mesh cell has the identity row already; table
    (count + 1, 6): the predicted rows, row 0 zeros; codes (rows, pitch) uint16: the predicted code plane."""
    R = padded_rows(A, b, nx)
    rows, pitch = R.shape[:2]
    # np.unique over axis 0 of an unsigned array sorts the rows lexicographically: the tie-break order as it stands
    uniq, inverse, counts = np.unique(bit_view(R).reshape(-1, 6), axis=0, return_inverse=True, return_counts=True)
    order = np.argsort(-counts.astype(np.int64), kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    table = np.zeros((len(uniq) + 1, 6))
    table[1:] = uniq[order].view(np.float64)
    codes = (rank[inverse.reshape(-1)] + 1) * 8
    assert codes.max() < 1 << 16 or len(uniq) >= LUT_MAX_ROWS
    return Model(len(uniq), table, (codes & 0xFFFF).astype(np.uint16).reshape(rows, pitch))


def rand_mask(rng, nx, ny, p=0.5):
    return np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8)


System = namedtuple("System", "A b D nx ny nimg K kind")


def base_system(oracle, nx, ny, nimg, seed, p=0.5):
    """The oracle's 2-phase system (Df 1, Ds 1e-2, walls 0 / 1) of `nimg` random masks with fluid fraction p, stacked."""
    rng = np.random.default_rng(seed)
    As, bs, Ds = [], [], []
    for _ in range(nimg):
        D = oracle.fill_D_2phase(rand_mask(rng, nx, ny, p), 1.0, 1e-2)
        A, b = oracle.discretize(D, 0.0, 1.0)
        As.append(A), bs.append(b), Ds.append(D)
    return np.concatenate(As), np.concatenate(bs), np.concatenate(Ds), rng


def designed_system(oracle, nx, ny, nimg, K, kind, seed, p=0.5):
    """A system with exactly K distinct rows (count_rows' count; K None: the base's own count): the base system, then new rows
    one cell at a time --
      kind "b"   sources b += k 2^-20, k = 1, 2, ..., in cells away from the wall columns (the dictionary then has b looked up
                 everywhere);
      kind "a0"  diagonals scaled by 1 + k 2^-30: the right-hand side stays on the walls, the matrix symmetric, positive definite
                 and diagonally dominant (a larger diagonal only), so conjugate gradients take it.
    Any other count than K is an AssertionError."""
    assert kind in ("b", "a0")
    A, b, D, rng = base_system(oracle, nx, ny, nimg, seed, p)
    A, b = A.copy(), b.copy()
    n = b.size
    census = Counter(bit_view(padded_rows(A, b, nx)).reshape(-1, 6).view("V48").ravel().tolist())
    if K is None:
        K = len(census)
    assert len(census) <= K, f"the base has {len(census)} rows already, more than K = {K}"
    col = np.arange(n) % nx
    cells = rng.permutation(np.flatnonzero((col > 0) & (col < nx - 1)) if kind == "b" else np.arange(n))
    k = 0
    for cell in cells:
        if len(census) == K:
            break
        k += 1
        old = bit_view(np.append(A[cell], b[cell])).tobytes()
        if kind == "b":
            b[cell] += k * 2.0 ** -20
        else:
            A[cell, 0] *= 1.0 + k * 2.0 ** -30
        census[old] -= 1
        if census[old] == 0:
            del census[old]
        census[bit_view(np.append(A[cell], b[cell])).tobytes()] += 1
    got = count_rows(A, b, nx).count
    assert got == K == len(census), f"built {got} rows (census {len(census)}), wanted {K}"
    return System(A, b, D, nx, ny, nimg, K, kind)


def uniform_D_system(oracle, nx, ny, seed):
    """Every cell its own diffusivity (uniform in 0.5 ... 2): every row of the system is its own."""
    D = np.random.default_rng(seed).uniform(0.5, 2.0, size=(ny, nx))
    A, b = oracle.discretize(D, 0.0, 1.0)
    return System(A, b, D, nx, ny, 1, None, "uniform")


def sparse_p(nx, ny):
    """fluid fraction of a mask with about four solid cells: its system has the nine position classes' rows and a few more"""
    return 1.0 - 4.0 / (nx * ny)


def near_equal_system(oracle, seed=40):
    """(system, changes): a K = 40 system of 64 x 40 (a mask with few solid cells: the base then has fewer than 40 rows) in
    which three single cells were changed so that the cell's new row and the row it had -- which other cells keep -- differ in
    one bit of a0, in one bit of aW, and in the sign of a zero b at a wall-column cell.  changes: (cell, plane) of each."""
    s = designed_system(oracle, 64, 40, 1, 40, "b", seed, p=sparse_p(64, 40))
    A, b = s.A.copy(), s.b.copy()
    R = bit_view(np.column_stack([A, b]))
    uniq, inverse, counts = np.unique(R, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    col = np.arange(b.size) % s.nx
    crowded = counts[inverse] >= 8                       # the row stays in the system after one cell leaves it
    inner = np.flatnonzero(crowded & (col > 1) & (col < s.nx - 2))
    wall = np.flatnonzero(crowded & (col == 0) & (R[:, 5] == 0))          # b = +0.0 there (CL = 0)
    assert len(inner) >= 2 and len(wall) >= 1
    c0, c1, c2 = int(inner[0]), int(inner[len(inner) // 2]), int(wall[0])
    assert A[c1, 1] != 0.0
    A[c0, 0] = np.nextafter(A[c0, 0], np.inf)
    A[c1, 1] = np.nextafter(A[c1, 1], 0.0)
    b[c2] = -0.0
    return System(A, b, s.D, s.nx, s.ny, 1, s.K + 3, "near"), [(c0, 0), (c1, 1), (c2, 5)]


def allb_pair(oracle, nx=260, ny=40, seed=260):
    """(clear, set, cell): a K = 511 "a0" system three strips of 128 columns wide -- its right-hand side lives on the walls --
    and the same system with one source in the middle strip, in a cell whose row was its own already (still 511 rows)."""
    if ("allb", nx, ny, seed) in _cache:
        return _cache[("allb", nx, ny, seed)]
    s = designed_system(oracle, nx, ny, 1, 511, "a0", seed)
    m = count_rows(s.A, s.b, nx)
    col = np.arange(s.b.size) % nx
    alone = np.bincount(m.codes.ravel() >> 3, minlength=m.count + 1)[m.codes.ravel() >> 3] == 1
    assert nx == 260
    cells = np.flatnonzero(alone & (col >= 128) & (col <= 131))     # columns that only a strip without a wall column can hold
    assert len(cells) >= 1
    cell = int(cells[len(cells) // 2])
    b = s.b.copy()
    b[cell] += 0.375
    t = System(s.A, b, s.D, nx, ny, 1, 511, "a0+source")
    assert count_rows(t.A, t.b, nx).count == 511
    _cache[("allb", nx, ny, seed)] = (s, t, cell)
    return s, t, cell


def sweeps_per_image(oracle, s, x0, n, **kw):
    """oracle.sweeps on every image of the stack"""
    m = s.nx * s.ny
    return np.concatenate([oracle.sweeps(s.A[k * m:(k + 1) * m], s.b[k * m:(k + 1) * m], x0[k * s.ny:(k + 1) * s.ny], n, **kw)
                           for k in range(s.nimg)])


# the cases of tests/test_gpu_dict.py; tests/test_dict_cases_host.py asserts every count on the CPU
SHAPES = [(64, 40, 1), (65, 41, 1), (130, 71, 1), (64, 40, 3)]
KS = [None, 33, 256, 510, 511]
KINDS = ["b", "a0"]


def seed_of(nx, ny, nimg, K, kind):
    return 1000 * nx + 10 * ny + nimg + (K or 0) * 7 + (1 if kind == "a0" else 0)


_cache = {}


def case(oracle, nx, ny, nimg, K, kind):
    """designed_system for a case of the tables above, built once per process and never changed by its users."""
    key = (nx, ny, nimg, K, kind)
    if key not in _cache:
        if K is not None and K < 90:
            # fewer rows than a half-and-half mask's base has (92 ... 97): a mask with few solid cells
            _cache[key] = designed_system(oracle, nx, ny, nimg, K, kind, seed_of(*key), p=sparse_p(nx, ny))
        else:
            _cache[key] = designed_system(oracle, nx, ny, nimg, K, kind, seed_of(*key))
        for a in _cache[key][:3]:
            a.setflags(write=False)
    return _cache[key]
