"""What a context holds AFTER deff_solve_stream returns (include/deff_amd.h at deff_solve_stream): slot k is an ordinary image
of the stack -- the last image that ran in it, the call's 2-phase system, that image's FINAL field; a slot that never received
an image holds zero rows and a zero field.  Every stream test elsewhere closes the context as soon as the stream returns.

The hazard: an image that stops while other slots keep sweeping stays frozen in the ping-pong buffer it stopped in.  Whether
that buffer is the one every later call reads depends on the parity of the buffer flips after its retirement -- one flip per
sweep on the single-sweep kernel, one per pass of T sweeps plus one per remaining sweep on the temporally blocked ones.  So
the cases run a stack with ONE early stopper (a parallel-stripes image: its Deff does not move after the first sweep, so it
stops at its second check whatever the tolerance) next to images that run to max_iter, for 16 consecutive values of
max_iter -- at least two whole passes of the longest pass (T = 8), so both parities occur whatever the pass length -- and then
use the context: read-back of the stack and of every slot, wall fluxes, residual, further sweeps and a further solve (the
oracle's bits from the oracle's fields), CG (its own honesty checks), and a second stream.  Everything against the CPU oracle
bit for bit."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cg import assert_fluxes_of_field, assert_honest

pytestmark = pytest.mark.gpu

DS, DF, CL, CR = 1e-2, 1.0, 0.25, 0.75
TOL, CE = 1e-6, 10                                           # the stripes stop at their second check: sweep CE + 1
MAX_ITERS = list(range(CE + 2, CE + 2 + 16))                 # 1 ... 16 sweeps of the others after the early stopper froze

# (kernel, tuning): the single-sweep kernel flips once per sweep; the blocked ones in both forms (1 streaming, 2 workgroup
# tiles), both launch modes (0 resident where the tiles fit, 1 one launch per pass) and two pass lengths
CONFIGS = [("matfree", {})] + [("matfree_tb", {"tb_impl": impl, "tb_launch": launch, "tb_T": T})
                               for impl in (1, 2) for launch in (0, 1) for T in (2, 8)]
TALL = ("matfree_tb", {"tb_impl": 2, "tb_launch": 0, "tb_T": 8, "tb_NW": 16})   # the tall 16-wave tiles, asked for by name
SHAPES = [(64, 48), (97, 41)]                                # an even and an odd width (padded rows on the device)
TALL_SHAPE = (256, 192)                                      # a size the tall tiles take (the smoke run's)
CASES = [(k, t, s) for (k, t) in CONFIGS for s in SHAPES] + [(TALL[0], TALL[1], TALL_SHAPE), (CONFIGS[6][0], CONFIGS[6][1], TALL_SHAPE)]


def case_id(c):
    k, t, (nx, ny) = c
    return "-".join([k] + [f"{a[3:]}{b}" for a, b in t.items()] + [f"{nx}x{ny}"])


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def make_images(nx, ny, B, seed=0):
    """B images; image 1 is the early stopper: parallel stripes (test_gpu_parity.py::test_streaming_batch_refills_slots).  Its
    wall fluxes, all the stopping rule looks at, do not move after the first sweep, so it stops at its second check whatever
    the tolerance; its field still changes from sweep to sweep (1e-4 between sweeps 10 and 11 on these meshes), so an older
    iterate is told from the final one."""
    rng = np.random.default_rng(1234 + seed)
    imgs = [np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8) for p in (0.45, 0.5, 0.6)[:B]]
    imgs[1][:] = 255
    imgs[1][:10, :] = 0                                      # parallel stripes
    return imgs


_ORACLE = {}


def oracle_run(ob, pix, max_iter):
    """(D, A, b, oracle.jacobi(...)) of one image from the linear guess; cached over the kernel configurations."""
    key = (pix.tobytes(), pix.shape, max_iter)
    if key not in _ORACLE:
        ny, nx = pix.shape
        D = ob.fill_D_2phase(pix, DF, DS)
        A, b = ob.discretize(D, CL, CR)
        _ORACLE[key] = (D, A, b, ob.jacobi(A, b, ob.linear_guess(nx, ny, CL, CR), D, CL, CR, TOL, max_iter, check_every=CE))
    return _ORACLE[key]


def open_solver(pkg, nx, ny, B, kernel, tune):
    s = pkg.Solver(nx, ny, nimg=B, kernel=kernel)
    for k, v in tune.items():
        s.set_tuning(k, v)
    return s


def slot_field(s, k):
    from effectivediffusivityfvm_amd import _capi
    x = np.empty((s.ny, s.nx))
    _capi.check(_capi.load().deff_get_slot_field(s._ctx, k, x))
    return x


def slot_residual(s, k):
    from effectivediffusivityfvm_amd import _capi
    r = C.c_double()
    _capi.check(_capi.load().deff_residual_slot(s._ctx, k, C.byref(r)))
    return r.value


def stream_and_check(s, ob, imgs, max_iter, tag):
    """One stream; every image's result and field against the oracle (asserted: this is what the stream tests elsewhere
    establish).  -> per slot (image, D, A, b, final field) of the last image the done callback reported for it."""
    B = s.nimg
    res = s.solve_stream(imgs, DS, DF, CL, CR, TOL, max_iter, check_every=CE, want_fields=True)
    assert len(res) == len(imgs)
    held = {}
    for i, pix in enumerate(imgs):
        D, A, b, (it, deff, conv, x, _, _) = oracle_run(ob, pix, max_iter)
        assert (res[i].iters, res[i].deff_raw, res[i].conv) == (it, deff, conv), (tag, max_iter, i, res[i])
        assert np.array_equal(res[i].field, x), (tag, max_iter, i)
        assert 0 <= res[i].slot < B
        held[res[i].slot] = (i, D, A, b, x)                  # images of one slot run one after the other: the later id is the last
    return res, held


def check_context(s, ob, held, max_iter, bad, tag):
    """Every reader of the context against the fields the model says it holds; mismatches are collected, not raised, so that
    one run shows every (max_iter, slot) that is wrong."""
    B, ny, nx = s.nimg, s.ny, s.nx
    got = s.get_field()
    d, MFL, MFR = s.flux()
    r = s.residual()
    for k in range(B):
        _, D, A, b, x = held[k]
        if not np.array_equal(got[k * ny:(k + 1) * ny], x):
            bad.append((tag, max_iter, k, "get_field"))
        if not np.array_equal(slot_field(s, k), x):
            bad.append((tag, max_iter, k, "get_slot_field"))
        want, L, R = ob.flux_deff(x, D, CL, CR)
        if not (d[k] == want and np.array_equal(MFL[k * ny:(k + 1) * ny], L) and np.array_equal(MFR[k * ny:(k + 1) * ny], R)):
            bad.append((tag, max_iter, k, "flux"))
        for name, val in (("residual", r[k]), ("residual_slot", slot_residual(s, k))):
            try:
                ob.assert_residual(val, x, D, CL, CR)
            except AssertionError:
                bad.append((tag, max_iter, k, name))


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_context_after_a_stream_with_one_early_stopper(pkg, oracle, case, B):
    """Before deff_solve_stream consolidated its slots on the way out, the early stopper's slot (slot 1) held its previous
    iterate whenever the buffer flips after its stop were odd in number: every reader below, and everything continued from
    it, was then wrong for that slot and that slot only, and nothing else in the suite noticed."""
    kernel, tune, (nx, ny) = case
    imgs = make_images(nx, ny, B)
    bad = []
    for max_iter in MAX_ITERS:
        want = [oracle_run(oracle, p, max_iter)[3] for p in imgs]
        # what the case rests on, from the oracle alone: the stripes stop at sweep CE + 1, the others run to max_iter
        assert [w[0] for w in want] == [max_iter, CE + 1, max_iter][:B]
        with open_solver(pkg, nx, ny, B, kernel, tune) as s:
            res, held = stream_and_check(s, oracle, imgs, max_iter, "first")
            assert sorted(held) == list(range(B))
            check_context(s, oracle, held, max_iter, bad, "after the stream")
            if "tb_NW" in tune:
                assert s.plan()["tb_NW"] == tune["tb_NW"], s.plan()
            # go on from there: 3 sweeps, then a solve that ends between two checks -- the oracle's bits from the oracle's fields
            s.sweeps(3)
            xs = [oracle.sweeps(held[k][2], held[k][3], held[k][4], 3) for k in range(B)]
            got = s.get_field()
            for k in range(B):
                if not np.array_equal(got[k * ny:(k + 1) * ny], xs[k]):
                    bad.append(("sweeps", max_iter, k, "get_field"))
            r2 = s.solve(1e-12, 7, check_every=3)
            got = s.get_field()
            for k in range(B):
                _, D, A, b, _ = held[k]
                it, deff, conv, x, _, _ = oracle.jacobi(A, b, xs[k], D, CL, CR, 1e-12, 7, check_every=3)
                if (r2[k].iters, r2[k].deff_raw, r2[k].conv) != (it, deff, conv) or not np.array_equal(got[k * ny:(k + 1) * ny], x):
                    bad.append(("solve", max_iter, k, "result / field"))
            assert s.plan_value("tb_fallbacks") == 0
        # a context of its own for what does not continue bit for bit: CG from the stream's fields, then a second stream
        with open_solver(pkg, nx, ny, B, kernel, tune) as s:
            res, held = stream_and_check(s, oracle, imgs, max_iter, "first")
            rc = s.solve_cg(rtol=1e-9, max_iter=100000)
            x = s.get_field()
            for k in range(B):
                _, D, A, b, x0 = held[k]
                assert rc[k].converged and rc[k].rel_residual <= 1e-9, (max_iter, k, rc[k])
                assert_honest(rc[k], 1e-9, A, b, x[k * ny:(k + 1) * ny], nx, ny)
            assert_fluxes_of_field(s, rc)
            # the same images again, in another order: what a fresh context gives (the oracle's numbers), and the slots follow
            again = imgs[::-1]
            res2, held2 = stream_and_check(s, oracle, again, max_iter, "second")
            check_context(s, oracle, held2, max_iter, bad, "after the second stream")
            assert s.plan_value("tb_fallbacks") == 0
    print(f"{case_id(case)} B={B}: {len(bad)} mismatches (sweeps after the early stop, slot)", sorted({(b[1] - CE - 1, b[2]) for b in bad})[:40])
    assert not bad, bad[:24]


@pytest.mark.parametrize("no_sweep", ["max_iter 0", "tol at the seed"])
def test_context_after_a_stream_that_never_sweeps(pkg, oracle, no_sweep):
    """max_iter <= 0, or a tolerance the seeded change (100, cuh:1173) already meets: no sweep runs, every image is reported
    with 0 sweeps, and the context holds the last B images with their linear guesses."""
    nx, ny, B = 97, 41, 2
    imgs = make_images(nx, ny, 3, seed=1)
    tol, max_iter = (1e-6, 0) if no_sweep == "max_iter 0" else (100.0, 50)
    with pkg.Solver(nx, ny, nimg=B) as s:
        res = s.solve_stream(imgs, DS, DF, CL, CR, tol, max_iter, check_every=CE, want_fields=True)
        assert [r.iters for r in res] == [0, 0, 0]
        x0 = oracle.linear_guess(nx, ny, CL, CR)
        held = {}
        for i, r in enumerate(res):
            assert np.array_equal(r.field, x0)
            held[r.slot] = i
        assert sorted(held) == [0, 1]
        got = s.get_field()
        d, MFL, MFR = s.flux()
        for k in range(B):
            assert np.array_equal(got[k * ny:(k + 1) * ny], x0)
            D = oracle.fill_D_2phase(imgs[held[k]], DF, DS)
            A, b = oracle.discretize(D, CL, CR)
            want, L, R = oracle.flux_deff(x0, D, CL, CR)
            assert d[k] == want and np.array_equal(MFL[k * ny:(k + 1) * ny], L)
        s.sweeps(5)
        got = s.get_field()
        for k in range(B):
            D = oracle.fill_D_2phase(imgs[held[k]], DF, DS)
            A, b = oracle.discretize(D, CL, CR)
            assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(A, b, x0, 5)), k


@pytest.mark.parametrize("kernel,tune", [CONFIGS[0], CONFIGS[2], CONFIGS[6], ("explicit", {})], ids=["matfree", "tb-streaming", "tb-tiles", "explicit"])
@pytest.mark.parametrize("count", [1, 2])
def test_fewer_images_than_slots(pkg, oracle, kernel, tune, count):
    """3 slots, 1 or 2 images: the unused slots read 0, their Deff and residual are finite, and the context takes a new
    image, assembly, guess and solve like any other."""
    nx, ny, B = 97, 41, 3
    imgs = make_images(nx, ny, 3, seed=2)[:count]
    max_iter = CE + 5
    with open_solver(pkg, nx, ny, B, kernel, tune) as s:
        # something else in every buffer first: the stream must not leave it behind in the slots it does not use
        rng = np.random.default_rng(7)
        s.set_image(np.stack(make_images(nx, ny, 3, seed=3)))
        s.assemble_2phase(1e-3, 2.0, 0.0, 1.0)
        s.set_field(rng.random((B * ny, nx)))
        s.sweeps(3)
        res = s.solve_stream(imgs, DS, DF, CL, CR, TOL, max_iter, check_every=CE, want_fields=True)
        used = {}
        for i, r in enumerate(res):
            D, A, b, (it, deff, conv, x, _, _) = oracle_run(oracle, imgs[i], max_iter)
            assert (r.iters, r.deff_raw, r.conv) == (it, deff, conv) and np.array_equal(r.field, x)
            used[r.slot] = (D, x)
        assert sorted(used) == list(range(count))
        got = s.get_field()
        d, MFL, MFR = s.flux()
        r = s.residual()
        for k in range(B):
            if k in used:
                D, x = used[k]
                assert np.array_equal(got[k * ny:(k + 1) * ny], x) and np.array_equal(slot_field(s, k), x), k
                assert d[k] == oracle.flux_deff(x, D, CL, CR)[0], k
                oracle.assert_residual(r[k], x, D, CL, CR)
            else:
                assert not got[k * ny:(k + 1) * ny].any() and not slot_field(s, k).any(), k
                assert np.isfinite(d[k]) and np.isfinite(r[k]) and np.isfinite(slot_residual(s, k)), (k, d[k], r[k])
                assert np.isfinite(MFL[k * ny:(k + 1) * ny]).all() and np.isfinite(MFR[k * ny:(k + 1) * ny]).all()
        # ... and the context goes on like any other
        pix = make_images(nx, ny, 3, seed=4)
        s.set_image(np.stack(pix))
        s.assemble_2phase(1e-3, 2.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        r3 = s.solve(1e-4, 57, check_every=10)
        got = s.get_field()
        for k in range(B):
            D = oracle.fill_D_2phase(pix[k], 2.0, 1e-3)
            A, b = oracle.discretize(D, 0.0, 1.0)
            it, deff, conv, x, _, _ = oracle.jacobi(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), D, 0.0, 1.0, 1e-4, 57, check_every=10)
            assert (r3[k].iters, r3[k].deff_raw, r3[k].conv) == (it, deff, conv), k
            assert np.array_equal(got[k * ny:(k + 1) * ny], x), k
        assert s.plan_value("tb_fallbacks") == 0


def test_stream_on_the_explicit_kernel_refills_its_coefficient_planes(pkg, oracle):
    """The explicit kernel reads coefficient planes, not codes: a slot that takes a new image needs that image's rows in them.
    5 images through 2 slots, every one against a one-image run of the reference loop, and the context afterwards."""
    nx, ny, B = 64, 48, 2
    rng = np.random.default_rng(31)
    imgs = [np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8) for p in (0.4, 0.5, 0.6, 0.45, 0.55)]
    imgs[0] = make_images(nx, ny, 2)[1]                      # slot 0 is refilled early
    for max_iter in (CE + 4, CE + 5):
        with pkg.Solver(nx, ny, nimg=B, kernel="explicit") as s:
            bad = []
            res, held = stream_and_check(s, oracle, imgs, max_iter, "explicit")
            check_context(s, oracle, held, max_iter, bad, "after the stream")
            assert not bad, bad
