"""deff_residual / deff_residual_slot / deff_residual_D where the residual kernels carry something (kernels_residual.hpp):
runs of several tiles per wave (kt > 1: two kept rows, the S face that becomes the next row's N face, the outer-neighbour
registers of lanes 0 and 63 reloaded per tile), ragged last runs and tiles, EDGE strips, all four <PHASES, FAST>
instantiations, per-image offsets of a stack, and both loops of k_residual_final.

Every case first asserts from deff_get_plan that the launch had the shape the case is there for -- "res_kt" (run length as
used: planner, tuning key, clip to the image's tile rows) and "res_items" (partial sums per image) -- then compares with the
oracle through oracle_binding.assert_residual (1e-13 of the per-cell doubles added in long double; max(1e-12, n * 2^-53) of
the serial sum) and asks for the same bits on a second call.  Expected plan values: strips = ceil(nx / 128), tile rows =
ceil(ny / 8), res_items = strips * ceil(tile rows / res_kt); deff_residual_D: ny * ceil(nx / 256)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CL, CR = 0.25, 0.75


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def plan_of(s):
    return s.plan_value("res_kt"), s.plan_value("res_items")


def check(s, oracle, plan, f, D, cl=CL, cr=CR):
    """One image: the plan of the call, the oracle, the same bits again.  Returns the value."""
    got = s.residual()
    assert plan_of(s) == plan, (plan_of(s), plan)
    oracle.assert_residual(got, f, D, cl, cr)
    assert s.residual() == got
    return got


def check_field_and_iterate(s, oracle, plan, f, D, cl=CL, cr=CR):
    """A random field, then the iterate after 9 sweeps from the linear guess (read back: the residual is what is tested)."""
    s.set_tuning("res_kt", plan[2])
    s.set_field(f)
    check(s, oracle, plan[:2], f, D, cl, cr)
    s.init_linear(cl, cr)
    s.sweeps(9)
    x = s.get_field()
    assert np.isfinite(x).all()
    check(s, oracle, plan[:2], x, D, cl, cr)


def slot_residual(s, k):
    from effectivediffusivityfvm_amd import _capi
    r = C.c_double()
    _capi.check(_capi.load().deff_residual_slot(s._ctx, k, C.byref(r)))
    return r.value


def mask_2phase(rng, ny, nx):
    return np.where(rng.random((ny, nx)) < 0.45, 0, 255).astype(np.uint8)


# (nx, ny, "res_kt" set) -> ("res_kt", "res_items") the plan must report
FORCED = [
    (130, 9, 2, 2, 2),        # second tile of the run has one row; EDGE strip of 2 columns
    (97, 41, 3, 3, 2),        # odd width (padded rows, not FAST); last run of 8 + 8 + 1 rows
    (257, 33, 64, 5, 3),      # clipped to the 5 tile rows; EDGE strip = one mesh column and the pad cell
    (258, 50, 2, 2, 12),      # even width (FAST), three strips; the last run is one ragged tile
    (1030, 37, 2, 2, 27),     # nine strips; last run of one 5-row tile
]


@pytest.mark.parametrize("nx,ny,set_kt,kt,items", FORCED)
def test_forced_runs_2phase(pkg, oracle, nx, ny, set_kt, kt, items):
    rng = np.random.default_rng(nx * 1000 + ny)
    pix = mask_2phase(rng, ny, nx)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        check_field_and_iterate(s, oracle, (kt, items, set_kt), rng.random((ny, nx)) * 3 - 1, D)


@pytest.mark.parametrize("nx,ny,set_kt,kt,items", [FORCED[1], FORCED[3]])
def test_forced_runs_3phase(pkg, oracle, nx, ny, set_kt, kt, items):
    """<3, false> and <3, true> with kt > 1: three pixel classes, impermeable solid (every face of a solid cell has
    conductance exactly 0), the system assembled with the flood-filled Grid."""
    rng = np.random.default_rng(nx * 1000 + ny + 3)
    pix = rng.choice(np.array([0, 30, 120, 199, 201, 255], dtype=np.uint8), size=(ny, nx), p=[0.25, 0.1, 0.25, 0.1, 0.1, 0.2])
    pix[0] = pix[-1] = 255        # as test_residual_3phase_with_impermeable_solid: FloodFill wraps top <-> bottom
    grid, _ = oracle.floodfill((pix > 200).astype(np.uint32))
    D = oracle.fill_D_3phase(pix, 1.0, 0.0, 50.0)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_3phase(0.0, 1.0, 50.0, CL, CR, grid=grid)
        check_field_and_iterate(s, oracle, (kt, items, set_kt), rng.random((ny, nx)) * 3 - 1, D)


@pytest.mark.parametrize("ampX,ampY", [(2, 1), (3, 2)])
def test_forced_runs_with_mesh_amplification(pkg, oracle, ampX, ampY):
    """258 x 50 as an amplified 129 x 50 / 86 x 25 image: an even mesh width on the instantiation that is not FAST, ny / ampY
    rows of pixels behind the runs."""
    nx, ny = 258, 50
    rng = np.random.default_rng(ampX * 10 + ampY)
    pix = mask_2phase(rng, ny // ampY, nx // ampX)
    D = oracle.fill_D_2phase(pix, 2.0, 1e-2, ampX, ampY)
    assert D.shape == (ny, nx)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix, ampX, ampY)
        s.assemble_2phase(1e-2, 2.0, CL, CR)
        check_field_and_iterate(s, oracle, (2, 12, 2), rng.random((ny, nx)) * 3 - 1, D)


def test_stack_runs_stay_inside_their_image(pkg, oracle):
    """5 x 250 x 90, runs of 4 tiles: 12 tile rows = 3 runs per strip and image, partial sums at per-image offsets.
    deff_residual_slot launches the same kernel on one image with nimg = 1: a wave's work item (image, strip, run) and its
    slot img * per_img + strip * cpi + run in the image's partial sums depend on the image's own shape and res_kt only, and
    k_residual_final adds one image's partial sums per workgroup -- so the slot call's value is the stacked call's, bit for
    bit."""
    nx, ny, B = 250, 90, 5
    rng = np.random.default_rng(250090)
    pix = np.stack([oracle.synth_mask(nx, ny, 77, k) for k in range(B)])
    Ds = [oracle.fill_D_2phase(pix[k], 1.0, 1e-3) for k in range(B)]
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        s.set_tuning("res_kt", 4)
        for iterate in (False, True):
            if iterate:
                s.init_linear(CL, CR)
                s.sweeps(9)
                f = s.get_field()
            else:
                f = rng.random((B * ny, nx)) * 3 - 1
                s.set_field(f)
            got = s.residual()
            assert plan_of(s) == (4, 6)
            assert got.shape == (B,)
            for k in range(B):
                oracle.assert_residual(got[k], f[k * ny:(k + 1) * ny], Ds[k], CL, CR)
            assert np.array_equal(s.residual(), got)
            for k in range(B):
                one = slot_residual(s, k)
                assert plan_of(s) == (4, 6)
                oracle.assert_residual(one, f[k * ny:(k + 1) * ny], Ds[k], CL, CR)
                assert one == got[k] and slot_residual(s, k) == one


def test_run_length_changes_only_the_order_of_the_sum(pkg, oracle):
    nx, ny = 258, 50
    rng = np.random.default_rng(25850)
    pix = mask_2phase(rng, ny, nx)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    f = rng.random((ny, nx)) * 3 - 1
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        s.set_field(f)
        got = []
        for kt, items in ((1, 21), (2, 12), (3, 9), (7, 3)):
            s.set_tuning("res_kt", kt)
            got.append(check(s, oracle, (kt, items), f, D))
    assert max(got) - min(got) <= 1e-13 * min(got), got


def test_the_planner_chooses_runs_for_a_stack_of_narrow_images(pkg, oracle):
    """Nothing forced: 130 images of 6 x 520 are 1 strip x 65 tile rows x 130 = 8450 work items, so the planner takes runs of
    8450 / 4096 = 2 tiles: 33 runs per image, the last one a single tile."""
    nx, ny, B = 6, 520, 130
    rng = np.random.default_rng(6520)
    pix = np.stack([oracle.synth_mask(nx, ny, 77, k) for k in range(B)])
    f = rng.random((B * ny, nx)) * 3 - 1
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        s.set_tuning("res_kt", 0)
        s.set_field(f)
        got = s.residual()
        assert plan_of(s) == (2, 33)
        again = s.residual()
    for k in range(B):
        oracle.assert_residual(got[k], f[k * ny:(k + 1) * ny], oracle.fill_D_2phase(pix[k], 1.0, 1e-3), CL, CR)
    assert np.array_equal(again, got)


def test_final_reduction_tail_and_four_load_loop(pkg, oracle):
    """k_residual_final, 1024 threads per image: 1917 partial sums (class kernel, res_kt 1: 9 strips x 213 tile rows) leave
    893 threads with two values in the tail loop and 131 with one; 8500 (deff_residual_D: 1700 rows x 5 segments) send every
    thread through the four-load loop twice and 308 threads through one more tail value."""
    nx, ny = 1030, 1700
    rng = np.random.default_rng(10301700)
    pix = mask_2phase(rng, ny, nx)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    f = rng.random((ny, nx)) * 3 - 1
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        s.set_tuning("res_kt", 1)
        s.set_field(f)
        got = s.residual()
        assert plan_of(s) == (1, 1917)
        again = s.residual()
        got_D = s.residual(D, CL, CR)
        assert plan_of(s) == (0, 8500)
        again_D = s.residual(D, CL, CR)
    oracle.assert_residual(got, f, D, CL, CR)
    oracle.assert_residual(got_D, f, D, CL, CR)
    assert again == got and again_D == got_D


def test_final_reduction_offsets_of_a_stack_through_the_plane_kernel(pkg, oracle):
    """2 x 1030 x 300 through deff_residual_D: image 1's partial sums start at blockIdx.x * per_img = 1500."""
    nx, ny, B = 1030, 300, 2
    rng = np.random.default_rng(1030300)
    pix = mask_2phase(rng, B * ny, nx)
    D = np.concatenate([oracle.fill_D_2phase(pix[k * ny:(k + 1) * ny], 1.0, 1e-3) for k in range(B)])
    f = rng.random((B * ny, nx)) * 3 - 1
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        s.set_field(f)
        got = s.residual(D, CL, CR)
        assert plan_of(s) == (0, 1500)
        assert np.array_equal(s.residual(D, CL, CR), got)
    for k in range(B):
        oracle.assert_residual(got[k], f[k * ny:(k + 1) * ny], D[k * ny:(k + 1) * ny], CL, CR)


SEAM_COLS = (0, 1, 126, 127, 128, 129, 255, 256, 257)


def seam_probes(pkg, oracle, nx, ny, set_kt, plan, rows, cols):
    """Walls 0, a zero field with one cell set to 1: only that cell and its up to four neighbours have a non-zero term, so a
    wrong or dropped face at a seam cannot hide in the mean over the other cells."""
    rng = np.random.default_rng(nx * 1000 + ny + 7)
    pix = mask_2phase(rng, ny, nx)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, 0.0, 0.0)
        s.set_tuning("res_kt", set_kt)
        for i in rows:
            for j in cols:
                f = np.zeros((ny, nx))
                f[i, j] = 1.0
                s.set_field(f)
                try:
                    check(s, oracle, plan, f, D, 0.0, 0.0)
                except AssertionError as e:
                    raise AssertionError(f"spike at row {i}, column {j}: {e}") from e


def test_seam_probes_258x50(pkg, oracle):
    """res_kt 2 on 7 tile rows: rows 0 / 49 the image's edges, 7 | 8 the tile seam inside a run, 15 | 16, 31 | 32 and 47 | 48 run
    seams (48, 49: the ragged last run); columns 0 / 257 the walls, 127 | 128 and 255 | 256 lane 63 | lane 0 between strips, 256 / 257 the EDGE
    strip."""
    seam_probes(pkg, oracle, 258, 50, 2, (2, 12), (0, 7, 8, 15, 16, 31, 32, 47, 48, 49), SEAM_COLS)


def test_seam_probes_257x33(pkg, oracle):
    """res_kt 64 clipped to 5: one run per strip, the last mesh column (256) next to the pad cell (257, which is not a mesh
    cell and cannot carry a spike); rows 0 and 32 the image's edges, 8 and 32 the first rows of a tile."""
    seam_probes(pkg, oracle, 257, 33, 64, (5, 3), (0, 8, 32), [j for j in SEAM_COLS if j < 257])


def test_plan_keys_of_the_residual(pkg, oracle):
    """0 / 0 before any residual call; a refused call leaves both as they were; deff_residual_D reports res_kt 0."""
    nx, ny = 130, 9
    rng = np.random.default_rng(1309)
    pix = mask_2phase(rng, ny, nx)
    D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_2phase(1e-3, 1.0, CL, CR)
        assert plan_of(s) == (0, 0)
        with pytest.raises(pkg.DeffError, match="no field"):
            s.residual()
        assert plan_of(s) == (0, 0)
        s.init_linear(CL, CR)
        s.residual()
        assert plan_of(s) == (1, 4)                               # the planner's run length: 2 strips x 2 tile rows
        s.assemble_from_D(D, CL, CR)                              # no pixel classes any more: deff_residual refuses
        with pytest.raises(pkg.DeffError, match="deff_residual_D"):
            s.residual()
        assert plan_of(s) == (1, 4)
        oracle.assert_residual(s.residual(D, CL, CR), oracle.linear_guess(nx, ny, CL, CR), D, CL, CR)
        assert plan_of(s) == (0, 9)
