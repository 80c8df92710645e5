"""The row dictionary harvest (csrc/kernels_dict.hpp, csrc/api_dict.hip) at its limits, read back and on every kernel that
reads it.  The systems come from tests/dict_cases.py, whose exact row counts tests/test_dict_cases_host.py asserts on the CPU;
the expected table and code plane are that module's host model of the code-order rule ("Row dictionary: code order").

  a  the harvest equals the model: outcome, row count, table, code plane, pad codes, expansion, a second context
  b  limits: 511 rows harvest and 512 do not; an odd width's pad row takes a seat; 2 560 rows; 20 480 rows overflow the hash table
  c  rows that differ in one bit of one plane, or in the sign of a zero
  d  a full table (511 rows + the zero row) through every sweep form and every CG form
  e  the right-hand side away from the walls (lut_allb), both ways, on a full table three strips wide"""
import warnings

import numpy as np
import pytest

import dict_cases as dc
import prescaled_model as pm
from test_cg_host import K_PARITY, pcg_numpy, rel_l2, residual_np
from test_gpu_cg import EPS, PARITY_M, assert_fluxes_of_field
from test_gpu_cg_planes import assert_same_bits, both_forms_agree, run as cg_run

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def last_error(pkg):
    return pkg._capi.load().deff_last_error().decode()


def context(pkg, s, kernel="auto", tune=None):
    c = pkg.Solver(s.nx, s.ny, nimg=s.nimg, kernel=kernel)
    for k, v in (tune or {}).items():
        c.set_tuning(k, v)
    c.set_system(s.A, s.b, s.D, 0.0, 1.0)
    return c


def field_of(s, seed=5):
    return np.random.default_rng(seed).random((s.nimg * s.ny, s.nx))


def assert_harvest_is_the_model(pkg, s, m):
    """One fresh context: set_system, sweeps(1) on kernel auto, then everything of (a).  Returns the code plane."""
    system = np.column_stack([s.A, s.b])
    with context(pkg, s) as c:
        assert c.plan_value("dict_outcome") == 0 and c.plan_value("dict_rows") == 0 and c.plan_value("lut_rows") == 0
        with pytest.raises(pkg.DeffError) as e:
            c.dictionary()
        assert e.value.code == ESTATE
        c.set_field(field_of(s))
        c.sweeps(1)
        assert c.plan_value("dict_outcome") == 1, c.plan_value("dict_outcome")
        assert c.plan_value("dict_rows") == m.count and c.plan_value("lut_rows") == m.count + 1
        assert c.kernel_in_use() == "matfree_tb"
        rows, codes = c.dictionary()
        assert rows.shape == m.table.shape and codes.shape == m.codes.shape
        assert np.array_equal(dc.bit_view(rows), dc.bit_view(m.table))
        assert np.array_equal(codes, m.codes)
        assert np.all(codes % 8 == 0) and codes.min() >= 8 and codes.max() == 8 * m.count
        if s.nx & 1:
            assert np.array_equal(rows[codes[:, s.nx] >> 3], np.broadcast_to(dc.IDENTITY, (codes.shape[0], 6)))
        back = rows[codes[:, :s.nx].astype(np.int64) >> 3].reshape(-1, 6)
        assert np.array_equal(dc.bit_view(back), dc.bit_view(system))
        A2, b2 = c.get_system()
        assert np.array_equal(dc.bit_view(A2), dc.bit_view(s.A)) and np.array_equal(dc.bit_view(b2), dc.bit_view(s.b))
        # read-only: a second read is the first, and the outcome stays
        rows2, codes2 = c.dictionary()
        assert np.array_equal(dc.bit_view(rows2), dc.bit_view(rows)) and np.array_equal(codes2, codes)
        assert c.plan_value("dict_outcome") == 1
        return codes


# ---------------------------------------------------------------------------------------------------------------------------
# a. The harvest equals the model

@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("K", dc.KS)
@pytest.mark.parametrize("nx,ny,nimg", dc.SHAPES)
def test_harvest_equals_the_model(pkg, oracle, nx, ny, nimg, K, kind):
    s = dc.case(oracle, nx, ny, nimg, K, kind)
    m = dc.count_rows(s.A, s.b, nx)
    assert m.count == s.K
    first = assert_harvest_is_the_model(pkg, s, m)
    second = assert_harvest_is_the_model(pkg, s, m)                   # a second fresh context: the same codes
    assert np.array_equal(first, second)


def test_a_priori_tables_read_back(pkg, oracle):
    """deff_get_dictionary on tables that were not harvested: the native 2-phase table (289 rows, pad cells carry the zero row)
    expands to the system get_system exports from the explicit planes; no harvest is recorded."""
    nx, ny = 65, 41
    pix = dc.rand_mask(np.random.default_rng(6541), nx, ny)
    A, b = oracle.discretize(oracle.fill_D_2phase(pix, 1.0, 1e-2), 0.0, 1.0)
    with pkg.Solver(nx, ny) as c:
        c.set_image(pix)
        c.assemble_2phase(1e-2, 1.0, 0.0, 1.0)
        rows, codes = c.dictionary()
        assert rows.shape == (289, 6) == (c.plan_value("lut_rows"), 6) and codes.shape == (ny, nx + 1)
        assert np.all(codes[:, nx] == 0) and np.all(rows[0] == 0)
        back = rows[codes[:, :nx].astype(np.int64) >> 3].reshape(-1, 6)
        assert np.array_equal(back, np.column_stack([A, b]))
        assert c.plan_value("dict_outcome") == 0 and c.plan_value("dict_rows") == 0


# ---------------------------------------------------------------------------------------------------------------------------
# b. Limits

def limit_system(oracle, name):
    if name == "even-512":
        return dc.case(oracle, 64, 40, 1, 512, "b"), 512, 2
    if name == "even-512-a0":
        return dc.case(oracle, 64, 40, 1, 512, "a0"), 512, 2
    if name == "odd-511-plus-pad":
        return dc.case(oracle, 65, 41, 1, 512, "b"), 512, 2
    if name == "2560-rows":
        return dc.uniform_D_system(oracle, 64, 40, 21), 2560, 2
    if name == "20480-rows-overflow":
        return dc.uniform_D_system(oracle, 160, 128, 22), 20480, 3
    raise KeyError(name)


def mesh_rows(s):
    return len(np.unique(dc.bit_view(np.column_stack([s.A, s.b])), axis=0))


def test_limit_harvested_full_tables(pkg, oracle):
    """Even width: 511 rows fill the table.  Odd width: 510 rows of the mesh and the pad column's identity row fill it."""
    s = dc.case(oracle, 64, 40, 1, 511, "b")
    assert mesh_rows(s) == 511
    with context(pkg, s) as c:
        c.set_field(field_of(s))
        c.sweeps(1)
        assert (c.plan_value("dict_outcome"), c.plan_value("dict_rows"), c.plan_value("lut_rows")) == (1, 511, 512)
    s = dc.case(oracle, 65, 41, 1, 511, "b")
    assert mesh_rows(s) == 510
    with context(pkg, s) as c:
        c.set_field(field_of(s))
        c.sweeps(1)
        assert (c.plan_value("dict_outcome"), c.plan_value("dict_rows"), c.plan_value("lut_rows")) == (1, 511, 512)
        rows, codes = c.dictionary()
        assert np.array_equal(rows[codes[0, 65] >> 3], dc.IDENTITY)


@pytest.mark.parametrize("name", ["even-512", "even-512-a0", "odd-511-plus-pad", "2560-rows", "20480-rows-overflow"])
def test_limit_refused_harvests(pkg, oracle, name):
    """One row too many (512 on an even width; 511 of the mesh + the pad row on an odd one), 2 560 rows, and 20 480 rows (more
    than the hash table's 16 384 slots): the outcome says which limit, and the system runs on the explicit planes."""
    s, count, outcome = limit_system(oracle, name)
    assert dc.count_rows(s.A, s.b, s.nx).count == count
    if name == "odd-511-plus-pad":
        assert mesh_rows(s) == 511
    x0 = field_of(s)
    want = oracle.sweeps(s.A, s.b, x0, 9)
    with context(pkg, s) as c:
        c.set_field(x0)
        assert c.plan_value("dict_outcome") == 0
        c.sweeps(9)
        assert c.plan_value("dict_outcome") == outcome and c.plan_value("dict_rows") == 0 and c.plan_value("lut_rows") == 0
        assert c.kernel_in_use() == "explicit"
        assert np.array_equal(c.get_field(), want)
        with pytest.raises(pkg.DeffError) as e:
            c.dictionary()
        assert e.value.code == ESTATE
        A2, b2 = c.get_system()
        assert np.array_equal(dc.bit_view(A2), dc.bit_view(s.A)) and np.array_equal(dc.bit_view(b2), dc.bit_view(s.b))
        # conjugate gradients: refused on the table form, the field as it was; taken on the coefficient planes
        c.init_linear(0.0, 1.0)
        x1 = c.get_field()
        c.set_tuning("cg_planes", 0)
        with pytest.raises(pkg.DeffError) as e:
            c.solve_cg(rtol=1e-10)
        assert e.value.code == EINVAL and "no row dictionary" in last_error(pkg)
        assert np.array_equal(c.get_field(), x1)
        c.set_tuning("cg_planes", 1)
        r = c.solve_cg(rtol=1e-10)
        assert r.converged and r.iters > 0 and c.plan_value("cg_impl") == 3
        res = residual_np(s.A, s.b, c.get_field(), s.nx, s.ny)
        assert res <= 1e-9, res
        assert c.plan_value("dict_outcome") == outcome                # one try per system: the refusal is remembered
        # a new system in the same context starts from "none tried"
        c.set_system(s.A, s.b, s.D, 0.0, 1.0)
        assert c.plan_value("dict_outcome") == 0


def test_limit_dictionaries_switched_off(pkg, oracle):
    s = dc.case(oracle, 64, 40, 1, 33, "b")
    x0 = field_of(s)
    with context(pkg, s, tune={"dict": 0}) as c:
        c.set_field(x0)
        c.sweeps(9)
        assert c.plan_value("dict_outcome") == 0 and c.plan_value("dict_rows") == 0
        assert c.kernel_in_use() == "explicit"
        assert np.array_equal(c.get_field(), oracle.sweeps(s.A, s.b, x0, 9))
        # switched back on, the same system is harvested at the next sweeps
        c.set_tuning("dict", 1)
        c.sweeps(1)
        assert c.plan_value("dict_outcome") == 1 and c.plan_value("dict_rows") == 33


# ---------------------------------------------------------------------------------------------------------------------------
# c. Near-equal rows

def test_near_equal_rows_keep_their_own_seats(pkg, oracle):
    """Rows one unit in the last place apart in a0 or aW, and rows whose only difference is b = -0.0 against +0.0, are
    different rows: 40 + 3, and the expansion gives every cell its own bits back."""
    s, changes = dc.near_equal_system(oracle)
    m = dc.count_rows(s.A, s.b, s.nx)
    assert m.count == 43
    codes = assert_harvest_is_the_model(pkg, s, m)
    flat = codes[:, :s.nx].ravel()
    for cell, plane in changes:
        assert (flat == flat[cell]).sum() == 1                        # a seat of its own
    x0 = field_of(s)
    with context(pkg, s) as c:
        c.set_field(x0)
        c.sweeps(9)
        assert c.kernel_in_use() == "matfree_tb"
        assert np.array_equal(c.get_field(), oracle.sweeps(s.A, s.b, x0, 9))


# ---------------------------------------------------------------------------------------------------------------------------
# d. A full table on every reader

FULL = [(130, 71, 1, "b"), (130, 71, 1, "a0"), (64, 40, 3, "b"), (64, 40, 3, "a0")]
FULL_IDS = [f"{nx}x{ny}x{B}-{kind}" for nx, ny, B, kind in FULL]
N_SWEEPS = 27
# name: (kernel, tuning keys, reference, plan keys the form must show)
SWEEP_FORMS = {
    "matfree": ("matfree", {}, "oracle", {}),
    "streaming-T2": ("matfree_tb", {"tb_impl": 1, "tb_T": 2}, "oracle", {"tb_impl": 1, "tb_T": 2}),
    "streaming-T8": ("matfree_tb", {"tb_impl": 1, "tb_T": 8}, "oracle", {"tb_impl": 1, "tb_T": 8}),
    "tiles-resident": ("matfree_tb", {"tb_impl": 2, "tb_T": 8, "tb_launch": 0}, "oracle", {"tb_impl": 2, "tb_T": 8, "tb_resident": 1}),
    "tiles-per-pass": ("matfree_tb", {"tb_impl": 2, "tb_T": 8, "tb_launch": 1}, "oracle", {"tb_impl": 2, "tb_T": 8, "tb_resident": 0}),
    # the tile families by name: the 8-wave tiles' table fill is sized for exactly 6 x 512 doubles
    "tiles-8-waves": ("matfree_tb", {"tb_impl": 2, "tb_T": 8, "tb_NW": 8}, "oracle", {"tb_impl": 2, "tb_T": 8, "tb_NW": 8}),
    "tiles-12-waves": ("matfree_tb", {"tb_impl": 2, "tb_T": 8, "tb_NW": 12}, "oracle", {"tb_impl": 2, "tb_T": 8, "tb_NW": 12}),
    "tiles-16-waves": ("matfree_tb", {"tb_impl": 2, "tb_T": 8, "tb_NW": 16}, "oracle", {"tb_impl": 2, "tb_T": 8, "tb_NW": 16}),
    "fma": ("auto", {"fma": 1}, "oracle-fma", {}),
    "prescaled": ("auto", {"prescaled": 1}, "prescaled-model", {"prescaled": 1}),
}
_wanted = {}


def wanted(oracle, s, key, reference):
    """The reference field of (system, arithmetic) after N_SWEEPS, computed once."""
    if (key, reference) not in _wanted:
        x0 = field_of(s)
        if reference == "prescaled-model":
            m = s.nx * s.ny
            w = np.concatenate([pm.sweeps(s.A[k * m:(k + 1) * m], s.b[k * m:(k + 1) * m], x0[k * s.ny:(k + 1) * s.ny], N_SWEEPS)
                                for k in range(s.nimg)])
        else:
            w = dc.sweeps_per_image(oracle, s, x0, N_SWEEPS, flavour="fma" if reference == "oracle-fma" else None)
        w.setflags(write=False)
        _wanted[(key, reference)] = w
    return _wanted[(key, reference)]


@pytest.mark.parametrize("form", list(SWEEP_FORMS))
@pytest.mark.parametrize("nx,ny,nimg,kind", FULL, ids=FULL_IDS)
def test_full_table_sweeps(pkg, oracle, nx, ny, nimg, kind, form):
    kernel, tune, reference, must = SWEEP_FORMS[form]
    s = dc.case(oracle, nx, ny, nimg, 511, kind)
    want = wanted(oracle, s, (nx, ny, nimg, kind), reference)
    with context(pkg, s, kernel=kernel, tune=tune) as c:
        c.set_field(field_of(s))
        c.sweeps(N_SWEEPS)
        assert c.plan_value("dict_outcome") == 1 and c.plan_value("lut_rows") == 512
        got = c.get_field()
        ran = {k: c.plan_value(k) for k in must}
        kern = c.kernel_in_use()
    # the bits hold for whatever form ran; a form the planner did not grant at this shape is named, not passed over
    assert np.array_equal(got, want), (form, kern, ran)
    assert kern == ("matfree_tb" if kernel == "auto" else kernel)
    if ran != must:
        warnings.warn(f"full table {nx}x{ny}x{nimg} {kind}: form '{form}' not granted by the planner: asked {must}, ran {ran}")


@pytest.mark.parametrize("nx,ny,nimg", [(130, 71, 1), (64, 40, 3)])
def test_full_table_conjugate_gradients(pkg, oracle, nx, ny, nimg):
    """The "a0" systems (symmetric, positive definite): the table form streaming and on chip, folded and not, against numpy's
    CG in long double under test_gpu_cg.py's bar M max(g(k), 4 eps); the table form against the plane form, the same bits."""
    s = dc.case(oracle, nx, ny, nimg, 511, "a0")
    m = nx * ny
    x0 = np.concatenate([oracle.linear_guess(nx, ny, 0.0, 1.0)] * nimg)
    imgs = [(s.A[k * m:(k + 1) * m], s.b[k * m:(k + 1) * m], x0[k * ny:(k + 1) * ny]) for k in range(nimg)]
    t64 = [pcg_numpy(A, b, x, nx, ny, K_PARITY, np.float64) for A, b, x in imgs]
    tld = [pcg_numpy(A, b, x, nx, ny, K_PARITY, np.longdouble) for A, b, x in imgs]
    with context(pkg, s) as c:
        for onchip in (0, 1):
            for fold in (0, 1, 2):
                c.set_tuning("cg_planes", 0), c.set_tuning("cg_onchip", onchip), c.set_tuning("cg_fold", fold)
                for k in K_PARITY:
                    c.set_field(x0)
                    rs = c.solve_cg(rtol=0.0, max_iter=k)
                    rs = rs if isinstance(rs, list) else [rs]
                    xk = c.get_field()
                    assert c.plan_value("cg_impl") == (2 if onchip else 1), (onchip, fold, c.plan_value("cg_impl"))
                    assert c.plan_value("cg_fold") == (0 if onchip else fold)
                    assert c.plan_value("dict_outcome") == 1 and c.plan_value("lut_rows") == 512
                    assert_fluxes_of_field(c, rs if nimg > 1 else rs[0])
                    for i, (A, b, _) in enumerate(imgs):
                        xi = xk[i * ny:(i + 1) * ny]
                        assert rs[i].iters == k and not rs[i].converged
                        res = residual_np(A, b, xi, nx, ny)
                        assert abs(rs[i].rel_residual - res) <= 1e-9 * res, (rs[i].rel_residual, res)
                        g = rel_l2(t64[i].fields[k], tld[i].fields[k])
                        gap = rel_l2(xi, tld[i].fields[k].astype(np.float64))
                        bar = PARITY_M * max(g, 4 * EPS)
                        print(f"full table {nx}x{ny}x{nimg} onchip {onchip} fold {fold} image {i} k={k}: g(k) {g:.3e} GPU gap {gap:.3e}")
                        assert gap <= bar, (onchip, fold, i, k, gap, g, bar)
        # the table form against the plane form: k iterations and a converged solve
        c.set_tuning("cg_onchip", 0)
        for fold in (0, 1, 2):
            c.set_tuning("cg_fold", fold)
            both_forms_agree(c, x0, rtol=0.0, max_iter=20)
            t = both_forms_agree(c, x0, rtol=1e-11, max_iter=20000)
            assert all(q[2] for q in t[0]), t[0]
        # ... and the on-chip form converges to the same tolerance (numpy's residual of its field, a decade of slack for
        # the recurrence's drift)
        c.set_tuning("cg_fold", 0)
        c.set_tuning("cg_onchip", 1)
        chip = cg_run(c, x0, 0, rtol=1e-11, max_iter=20000)
        assert chip[4] == 2 and all(q[2] for q in chip[0]), chip[0]
        for i, (A, b, _) in enumerate(imgs):
            assert residual_np(A, b, chip[2][i * ny:(i + 1) * ny], nx, ny) <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------------
# e. lut_allb

ALLB_FORMS = ["auto", "matfree", "streaming-T2", "streaming-T8", "tiles-resident", "tiles-8-waves", "prescaled"]


@pytest.mark.parametrize("form", ALLB_FORMS)
def test_right_hand_side_away_from_the_walls_on_a_full_table(pkg, oracle, form):
    """260 columns: three strips of 128, the middle one without a wall column -- it looks b up only when the harvest says some
    row away from the walls has one.  The same full table with and without one source in the middle strip: each equals the
    oracle, and the two differ (so the second run's source was read)."""
    clear, source, cell = dc.allb_pair(oracle)
    kernel, tune, reference, must = SWEEP_FORMS[form] if form != "auto" else ("auto", {}, "oracle", {})
    got = []
    for name, s in (("clear", clear), ("source", source)):
        want = wanted(oracle, s, ("allb", name), reference)
        with context(pkg, s, kernel=kernel, tune=tune) as c:
            c.set_field(field_of(s))
            c.sweeps(N_SWEEPS)
            assert c.plan_value("dict_outcome") == 1 and c.plan_value("dict_rows") == 511
            if kernel != "matfree" and c.plan_value("tb_impl") == 1:
                assert c.plan_value("tb_strips") >= 3, c.plan()
            ran = {k: c.plan_value(k) for k in must}
            got.append(c.get_field())
        assert np.array_equal(got[-1], want), (form, name, ran)
        if ran != must:
            warnings.warn(f"lut_allb 260x40 {name}: form '{form}' not granted by the planner: asked {must}, ran {ran}")
    i, j = divmod(cell, clear.nx)
    differ = got[0] != got[1]
    cols = differ.any(axis=0).nonzero()[0]
    assert differ[i, j] and cols.min() >= j - N_SWEEPS and cols.max() <= j + N_SWEEPS   # the source's reach: one cell per sweep
    # ... from a column that no wall strip can hold: a strip with column 0 ends by 127, one with column 259 starts from 132
    assert 128 <= j <= 131
    w0, w1 = wanted(oracle, clear, ("allb", "clear"), reference), wanted(oracle, source, ("allb", "source"), reference)
    assert np.array_equal(got[1] - got[0], w1 - w0)
