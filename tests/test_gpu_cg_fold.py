"""deff_solve_cg / deff_solve_cg_stream with the tuning key "cg_fold" (kernels_cg_fold.hpp): an iteration in two launches, the
per-image sums taken by the image's last workgroup to arrive.  The contract is the bits of key 0 -- fields, iteration counts,
residuals, Deff, wall fluxes and plans -- for every system, stack, check_every and call order; one stale or missing partial
sum changes them within an iteration or two.  Every test compares keys 1 and 2 with key 0 on one context from one guess and
asserts, from deff_get_plan, the geometry the shape was chosen for and the fold that ran."""
import numpy as np
import pytest

from test_cg_host import RESTART_CASE
from test_gpu_cg import RTOL_PARITY
from test_gpu_cg_planes import assert_same_bits, bits, dictionary_system, per_cell_system, run

pytestmark = pytest.mark.gpu

FOLDS = (1, 2)


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def geometry(nx, ny):
    """(cg_kr, cg_strips, cg_items) of an image: strips of 128 columns of the even pitch, ~8 192 items, 2..16 rows each."""
    ntx = -(-((nx + 1) & ~1) // 128)
    kr = max(2, min(16, ntx * ny // 8192))
    return kr, ntx, ntx * -(-ny // kr)


def run_fold(s, x0, fold, planes=0, **kw):
    """run() of test_gpu_cg_planes.py under cg_fold = fold, and the fold that ran."""
    s.set_tuning("cg_fold", fold)
    t = run(s, x0, planes, **kw)
    return t, s.plan_value("cg_fold")


def by_bits(t):
    """A run with its floats as bytes: a NaN (Deff of a system with CL = CR) equals itself."""
    return ([tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in q) for q in t[0]],) + tuple(t[1:])


def folds_agree(s, x0, planes=0, folds=FOLDS, **kw):
    """Keys 1 and 2 against key 0; the reference run."""
    ref, f0 = run_fold(s, x0, 0, planes, **kw)
    assert f0 == 0 and ref[4] == (3 if planes else 1), (f0, ref[4])
    assert ref[3][:3] == geometry(s.nx, s.ny), (ref[3], geometry(s.nx, s.ny))
    for fold in folds:
        t, f = run_fold(s, x0, fold, planes, **kw)
        assert f == (min(fold, 1) if planes else fold) and t[4] == ref[4], (fold, f, t[4])   # on planes 2 means 1
        assert_same_bits(by_bits(ref), by_bits(t))
    return ref


def check_fold_bits(s, x0, planes=0, folds=FOLDS, exact_iters=True):
    for k in (1, 2, 5, 20):
        for ce in (1, 7, 64):
            t = folds_agree(s, x0, planes, folds, rtol=0.0, max_iter=k, check_every=ce)
            if exact_iters:
                assert all(b[0] == k for b in t[0]), t[0]
    ref = None
    for ce in (1, 7, 64):
        t = folds_agree(s, x0, planes, folds, rtol=1e-13, max_iter=20000, check_every=ce)
        if ref is None:
            ref = t
        assert_same_bits(ref, t)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Bits on single images.  (nx, ny) -> (kr, strips, items): 2 x 2 one item (three idle waves must reach the barrier),
# 130 x 71 two strips and 18 workgroups, 258 x 9 15 items (the last workgroup is short), 514 x 101 64 workgroups

SHAPES = {(2, 2): (2, 1, 1), (3, 5): (2, 1, 3), (40, 32): (2, 1, 16), (33, 21): (2, 1, 11), (130, 71): (2, 2, 72),
          (258, 9): (2, 3, 15)}


@pytest.mark.parametrize("nx,ny", list(SHAPES), ids=[f"{a}x{b}" for a, b in SHAPES])
def test_fold_gives_the_bits_of_four_launches(pkg, oracle, nx, ny):
    assert geometry(nx, ny) == SHAPES[(nx, ny)]
    s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
    with s:
        ref = check_fold_bits(s, x0)
        assert ref[0][0][0] > 0


def test_fold_ten_thousand_iterations(pkg, oracle):
    """514 x 101 to rtol 1e-13: 64 workgroups, thousands of iterations -- thousands of chances for a stale partial."""
    nx, ny = 514, 101
    assert geometry(nx, ny) == (2, 5, 255)
    s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
    with s:
        ref = folds_agree(s, x0, rtol=1e-13, max_iter=200000)
        print("514 x 101:", ref[0], "restarts", ref[3][3])
        assert ref[0][0][0] > 1000


# ---------------------------------------------------------------------------------------------------------------------------
# 2. Other systems

OTHER_SYSTEMS = [(name, nx, ny) for name in ("from_D-4-levels", "sources-inside", "3phase-grid") for nx, ny in ((130, 71), (97, 41))]


@pytest.mark.parametrize("name,nx,ny", OTHER_SYSTEMS)
def test_fold_bits_on_other_systems(pkg, oracle, name, nx, ny):
    s, x0 = dictionary_system(pkg, oracle, name, nx, ny)
    with s:
        check_fold_bits(s, x0)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. Stacks.  (nx, ny, B) -> items per image: 10 (workgroups straddle images), 70, 1 (a workgroup finishes four images),
# 3 (a workgroup holds the last items of two images)

STACKS = {(33, 20, 3): 10, (130, 69, 5): 70, (2, 2, 7): 1, (3, 5, 6): 3}


def stack_images(oracle, nx, ny, B):
    """B different images.  The tiny ones are drawn here: one all fluid (the linear guess is its solution), the others mixed."""
    if nx * ny > 100:
        return np.stack([oracle.synth_mask(nx, ny, 12345, k) for k in range(B)])
    rng = np.random.default_rng(100 * nx + ny)
    imgs = []
    while len(imgs) < B:
        pix = (rng.integers(0, 2, (ny, nx)) * 255).astype(np.uint8)
        if len(imgs) == 0:
            pix[:] = 0
        if not any(np.array_equal(pix, q) for q in imgs) and (len(imgs) == 0 or 0 < pix.sum() < 255 * nx * ny):
            imgs.append(pix)
    return np.stack(imgs)


@pytest.mark.parametrize("nx,ny,B", list(STACKS), ids=[f"{b}x({a}x{c})" for a, c, b in STACKS])
def test_fold_bits_on_stacks(pkg, oracle, nx, ny, B):
    imgs = stack_images(oracle, nx, ny, B)
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_image(imgs)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        ref = check_fold_bits(s, x0, exact_iters=nx * ny > 100)
        assert s.plan_value("cg_items") == STACKS[(nx, ny, B)]
        iters = [b[0] for b in ref[0]]
        print(f"{B} x ({nx} x {ny}): iterations {iters}")
        assert len(set(iters)) > 1, iters                            # frozen images stop ticking next to running ones


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Plane form

def test_fold_on_planes_native(pkg, oracle):
    s, x0 = dictionary_system(pkg, oracle, "native", 130, 71)
    with s:
        check_fold_bits(s, x0, planes=2)


def test_fold_on_planes_stack(pkg, oracle):
    s, x0 = dictionary_system(pkg, oracle, "native", 33, 20, nimg=3)
    with s:
        ref = check_fold_bits(s, x0, planes=2)
        assert s.plan_value("cg_items") == 10 and len({b[0] for b in ref[0]}) > 1


@pytest.mark.parametrize("case", ["uniform-130x71", "log-97x41"])
def test_fold_on_planes_without_a_dictionary(pkg, oracle, case):
    """A per-cell D drawn cell by cell: no dictionary, cg_planes 1 takes the plane form."""
    s, nx, ny, D, CL, CR = per_cell_system(pkg, oracle, case)
    with s:
        x0 = s.get_field()
        for kw in (dict(rtol=0.0, max_iter=20, check_every=7), dict(rtol=RTOL_PARITY, check_every=64)):
            ref = folds_agree(s, x0, planes=1, **kw)
            assert ref[4] == 3
        assert ref[0][0][2] and ref[0][0][0] > 20


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Stop paths and call order

def native(pkg, oracle, nx, ny, Ds=1e-3, CL=0.0, CR=1.0):
    s = pkg.Solver(nx, ny)
    s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
    s.assemble_2phase(Ds, 1.0, CL, CR)
    s.init_linear(CL, CR)
    return s


def test_fold_stop_paths(pkg, oracle):
    nx, ny = 130, 71
    with native(pkg, oracle, nx, ny) as s:
        x0 = s.get_field()
        # max_iter 0
        ref = folds_agree(s, x0, rtol=1e-10, max_iter=0)
        assert ref[0][0][0] == 0 and not ref[0][0][2]
        # a converged start: 0 iterations, the field unchanged
        ref = folds_agree(s, x0, rtol=1e-10)
        assert ref[0][0][2] and ref[0][0][0] > 0
        again = folds_agree(s, ref[2], rtol=1e-10)
        assert again[0][0][0] == 0 and again[0][0][2] and np.array_equal(again[2], ref[2])
    # b = 0
    with native(pkg, oracle, nx, ny, CL=0.0, CR=0.0) as s:
        ref = folds_agree(s, np.zeros((ny, nx)), rtol=1e-10)
        assert ref[0][0][0] == 0 and ref[0][0][2] and np.all(ref[2] == 0.0)
    # every row decoupled
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(np.zeros((ny, nx)), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        ref = folds_agree(s, s.get_field(), rtol=1e-10)
        assert ref[0][0][0] == 0 and ref[0][0][2] and np.all(ref[2] == 0.0)


def test_fold_restart_round(pkg, oracle):
    nx, ny, Ds, rtol = RESTART_CASE
    with native(pkg, oracle, nx, ny, Ds=Ds) as s:
        ref = folds_agree(s, s.get_field(), rtol=rtol)
        assert ref[3][3] >= 1, ref[3]


def test_fold_call_order(pkg, oracle):
    """The same call twice, the keys alternating on one context, and a call that ends by max_iter in the middle of a check
    interval (the interval's frozen rest must leave no counter behind) followed by another call."""
    nx, ny = 130, 71
    with native(pkg, oracle, nx, ny) as s:
        x0 = s.get_field()
        first = {}
        for fold in (1, 1, 0, 2, 1, 0, 2, 2):
            t, f = run_fold(s, x0, fold, rtol=1e-11, check_every=7)
            assert f == fold
            first.setdefault(fold, t)
            assert_same_bits(first[fold], t)
            assert_same_bits(first[1], t)
        want = None
        for fold in (0, 1, 2, 1):
            s.set_tuning("cg_fold", fold)
            s.set_field(x0)
            a = s.solve_cg(rtol=0.0, max_iter=5, check_every=64)
            xa = s.get_field()
            b = s.solve_cg(rtol=1e-11, check_every=64)
            got = (bits(a), xa, bits(b), s.get_field())
            assert a.iters == 5 and b.converged and s.plan_value("cg_fold") == fold
            want = want or got
            assert got[0] == want[0] and got[2] == want[2]
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Large geometry

def test_fold_large(pkg):
    """2050 x 1537: kr 3, 17 strips, 2 181 workgroups -- several per compute unit, the last item one row."""
    nx, ny = 2050, 1537
    assert geometry(nx, ny) == (3, 17, 8721)
    with pkg.Solver(nx, ny) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        ref = folds_agree(s, s.get_field(), rtol=0.0, max_iter=50)
        assert ref[0][0][0] == 50


# ---------------------------------------------------------------------------------------------------------------------------
# 7. Stream

def stream(pkg, imgs, B, fold, on=0, ce=16):
    H, W = imgs[0].shape
    with pkg.Solver(W, H, nimg=B) as s:
        s.set_tuning("cg_onchip", on)
        s.set_tuning("cg_fold", fold)
        res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, rtol=1e-10, check_every=ce, want_fields=True)
        return res, {k: s.plan_value(k) for k in ("cg_impl", "cg_fold", "cgs_launches", "cgs_intervals", "cg_restarts")}


def assert_same_stream(a, b):
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert (p.iters, p.rel_residual, p.deff_raw, p.converged, p.slot) == (q.iters, q.rel_residual, q.deff_raw, q.converged, q.slot), k
        assert np.array_equal(p.field, q.field), k


@pytest.mark.parametrize("nx,ny,count,B", [(33, 20, 8, 3), (130, 69, 6, 2)], ids=["8x(33x20)-3-slots", "6x(130x69)-2-slots"])
def test_fold_in_a_stream(pkg, oracle, nx, ny, count, B):
    ce = 16
    imgs = [oracle.synth_mask(nx, ny, 777, k) for k in range(count)]
    want, p0 = stream(pkg, imgs, B, 0, ce=ce)
    assert (p0["cg_impl"], p0["cg_fold"]) == (1, 0) and all(r.converged for r in want)
    assert len({r.iters for r in want}) > 1
    for fold in FOLDS:
        got, p = stream(pkg, imgs, B, fold, ce=ce)
        assert (p["cg_impl"], p["cg_fold"]) == (1, fold)
        assert_same_stream(want, got)
        assert p["cgs_intervals"] == p0["cgs_intervals"] and p["cg_restarts"] == p0["cg_restarts"]
        saved = p0["cgs_launches"] - p["cgs_launches"]
        print(f"{count} x ({nx} x {ny}), fold {fold}: launches {p0['cgs_launches']} -> {p['cgs_launches']}")
        assert saved > 0 and saved % (2 * ce) == 0, (p0, p)


def test_fold_leaves_the_on_chip_stream_alone(pkg, oracle):
    imgs = [oracle.synth_mask(40, 32, 777, k) for k in range(7)]
    want, p0 = stream(pkg, imgs, 3, 0, on=1)
    got, p = stream(pkg, imgs, 3, 1, on=1)
    assert (p0["cg_impl"], p0["cg_fold"]) == (2, 0) and (p["cg_impl"], p["cg_fold"]) == (2, 0)
    assert_same_stream(want, got)
    assert p == p0
    # and deff_solve_cg on chip
    s, x0 = dictionary_system(pkg, oracle, "native", 40, 32)
    with s:
        s.set_tuning("cg_onchip", 1)
        ref, f0 = run_fold(s, x0, 0, rtol=1e-10)
        t, f = run_fold(s, x0, 2, rtol=1e-10)
        assert (ref[4], f0, t[4], f) == (2, 0, 2, 0)
        assert_same_bits(ref, t)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. Refusals

def test_cg_fold_takes_zero_one_or_two(pkg):
    with pkg.Solver(40, 32) as s:
        assert s.plan_value("cg_fold") == 0                          # before any call
        with pytest.raises(pkg.DeffError) as ei:
            s.set_tuning("cg_fold", 3)
        assert ei.value.code == -1
        for v in (0, 1, 2):
            s.set_tuning("cg_fold", v)


def test_fold_has_no_effect_on_row_slabs(pkg, oracle):
    nx, ny = 130, 71
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    got = []
    for fold in (0, 1):
        with pkg.SlabGroup(nx, ny, [0, 0, 0]) as g:
            g.set_image(pix)
            g.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            g.init_linear(0.0, 1.0)
            g.set_tuning("cg_fold", fold)
            r = g.solve_cg(rtol=1e-10)
            assert r.converged and g.plan_value(0, "cg_fold") == 0 and g.plan_value(0, "cg_impl") == 1
            got.append(((r.iters, r.rel_residual, r.deff_raw), g.get_field(), r.MFL.copy(), r.MFR.copy()))
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][1:], got[1][1:]):
        assert np.array_equal(a, b)
