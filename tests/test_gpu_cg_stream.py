"""deff_solve_cg_stream on the GPU: conjugate gradients through refilled slots (api_cg.hip, kernels_cg_stream.hpp).

The claim under test is one sentence of include/deff_amd.h: every image is solved exactly as a one-image deff_solve_cg call
would solve it from the linear guess -- so the reference of nearly every case is that call, given the same pixels through
set_image, and the comparison is bit for bit: (iters, rel_residual, deff_raw, converged) and the field `done` hands out.
The one-image runs are computed once per (image, settings) and shared (`one_image`).  Images come from
oracle.synth_mask(nx, ny, seed, k); settings are Ds 1e-3, Df 1, walls 0 / 1, rtol 1e-10 unless a case says otherwise."""
import ctypes as C
import json
import subprocess
import time

import numpy as np
import pytest

from test_cg_host import RESTART_CASE
from test_gpu_cg import DEFF_TOL, EXE
from test_gpu_cg_onchip import onchip

pytestmark = pytest.mark.gpu

SEED = 12345


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


def bits(r):
    return (r.iters, r.rel_residual, r.deff_raw, r.converged)


_ONE = {}


def one_image(pkg, pix, on=1, Ds=1e-3, rtol=1e-10, max_iter=1_000_000, amp=(1, 1)):
    """(bits, field, cg_impl, restart rounds) of a one-image context given `pix`; cached."""
    key = (pix.tobytes(), pix.shape, on, Ds, rtol, max_iter, amp)
    if key not in _ONE:
        H, W = pix.shape
        with onchip(pkg, W * amp[0], H * amp[1], on=on) as s:
            s.set_image(pix, amp[0], amp[1])
            s.assemble_2phase(Ds, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            r = s.solve_cg(rtol=rtol, max_iter=max_iter)
            x = s.get_field()
            x.setflags(write=False)
            _ONE[key] = (bits(r), x, s.plan_value("cg_impl"), s.plan_value("cg_restarts"))
    return _ONE[key]


def masks(oracle, nx, ny, count, first=0):
    return [oracle.synth_mask(nx, ny, SEED, first + k) for k in range(count)]


def run_stream(pkg, imgs, B, on=1, Ds=1e-3, rtol=1e-10, max_iter=1_000_000, ce=64, amp=(1, 1)):
    H, W = imgs[0].shape
    with onchip(pkg, W * amp[0], H * amp[1], nimg=B, on=on) as s:
        res = s.solve_cg_stream(imgs, Ds, 1.0, 0.0, 1.0, rtol=rtol, max_iter=max_iter, check_every=ce, want_fields=True,
                                ampX=amp[0], ampY=amp[1])
        return res, s.plan_value("cg_impl"), s.plan_value("cg_restarts")


def assert_one_image_bits(pkg, imgs, res, impl, **kw):
    assert len(res) == len(imgs)
    for k, (pix, r) in enumerate(zip(imgs, res)):
        want, x, impl1, _ = one_image(pkg, pix, **kw)
        assert impl1 == impl, (k, impl1, impl)
        assert bits(r) == want, (k, bits(r), want)
        assert np.array_equal(r.field, x), k


# ---------------------------------------------------------------------------------------------------------------------------
# 1. The bits of a one-image context

# the smallest shapes at which the pair mapping (2 x 2: one pair per row), the pad column (33), the whole register file
# (128 x 128 = all 16 384 cells), several 128-column strips with a ragged last one (258) or the slot list can go wrong
SHAPES = [(40, 32), (33, 21), (2, 2), (128, 128), (258, 9)]


@pytest.mark.parametrize("nx,ny", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_stream_gives_the_bits_of_one_image_contexts(pkg, oracle, nx, ny):
    """11 images through 3 slots: every slot is refilled several times, next to neighbours at other points of their solves."""
    imgs = masks(oracle, nx, ny, 11)
    first = None
    for ce in (64, 1, 7, 1000):
        res, impl, _ = run_stream(pkg, imgs, 3, ce=ce)
        assert impl == 2
        assert_one_image_bits(pkg, imgs, res, 2)
        assert all(0 <= r.slot < 3 for r in res) and {r.slot for r in res} == {0, 1, 2}
        got = [bits(r) for r in res]
        first = first or got
        assert got == first, ce
    assert len({b[0] for b in first}) > 1, first                     # or no slot ever outlives its neighbour
    assert all(b[3] for b in first)


def test_more_slots_than_compute_units(pkg, oracle):
    """400 images of 40 x 32 through 300 slots: workgroups of the on-chip launch take several slots, the lists are long, and
    every slot is refilled at most once."""
    imgs = masks(oracle, 40, 32, 400)
    res, impl, _ = run_stream(pkg, imgs, 300)
    assert impl == 2
    assert_one_image_bits(pkg, imgs, res, 2)
    per_slot = np.bincount([r.slot for r in res], minlength=300)
    assert per_slot.max() <= 2 and per_slot.min() >= 1 and per_slot.sum() == 400
    assert len({r.iters for r in res}) > 1


@pytest.mark.parametrize("nx,ny,on", [(40, 32, 0), (130, 130, 1)], ids=["40x32-key0", "130x130-too-large"])
def test_streaming_form(pkg, oracle, nx, ny, on):
    """The four streaming kernels iterate (cg_impl 1): without the key, and with it above 16 384 cells.  7 images, 3 slots."""
    imgs = masks(oracle, nx, ny, 7)
    first = None
    for ce in (64, 5):
        res, impl, _ = run_stream(pkg, imgs, 3, on=on, ce=ce)
        assert impl == 1
        assert_one_image_bits(pkg, imgs, res, 1, on=on)
        got = [bits(r) for r in res]
        first = first or got
        assert got == first, ce
    assert len({b[0] for b in first}) > 1 and all(b[3] for b in first)


def test_mesh_amplification(pkg, oracle):
    """20 x 11 pixels on a 40 x 33 mesh: the entry kernel's nearest-neighbour amplification against deff_set_image's."""
    imgs = masks(oracle, 20, 11, 7)
    res, impl, _ = run_stream(pkg, imgs, 3, amp=(2, 3))
    assert impl == 2 and res[0].field.shape == (33, 40)
    assert_one_image_bits(pkg, imgs, res, 2, amp=(2, 3))
    assert len({r.iters for r in res}) > 1


def test_ds_zero(pkg, oracle):
    """A solid that cannot diffuse: its rows are decoupled, x = 0 there exactly, and the fields are finite."""
    imgs = masks(oracle, 40, 32, 7)
    res, impl, _ = run_stream(pkg, imgs, 3, Ds=0.0)
    assert impl == 2
    assert_one_image_bits(pkg, imgs, res, 2, Ds=0.0)
    for pix, r in zip(imgs, res):
        assert np.all(np.isfinite(r.field))
        assert (pix >= 150).any() and np.all(r.field[pix >= 150] == 0.0)


def test_restart_rounds_inside_a_stream(pkg, oracle):
    """RESTART_CASE (contrast 1e6 at rtol 1e-14: the recurrence's residual reaches rtol before b - A x does) among other
    images of its size: it is sent back into the iteration while its neighbours run, and gives the one-image call's bits; the
    neighbours give the bits of a stream without it."""
    nx, ny, Ds, rtol = RESTART_CASE
    kw = dict(Ds=Ds, rtol=rtol, max_iter=200000)
    others = masks(oracle, nx, ny, 3, first=1)
    case = oracle.synth_mask(nx, ny, SEED, 0)
    want, _, impl1, rounds1 = one_image(pkg, case, **kw)
    assert impl1 == 2 and rounds1 >= 1 and want[3], (want, rounds1)
    with_it = [others[0], others[1], case, others[2]]
    res, impl, rounds = run_stream(pkg, with_it, 2, **kw)
    assert impl == 2 and rounds >= rounds1
    assert_one_image_bits(pkg, with_it, res, 2, **kw)
    res0, _, _ = run_stream(pkg, others, 2, **kw)
    for a, b in zip([res[0], res[1], res[3]], res0):
        assert bits(a) == bits(b) and np.array_equal(a.field, b.field)


def test_flux_reduce_tree(pkg, oracle):
    """"flux_reduce" 2: the slot's Deff is summed by k_flux_sum<true>'s butterfly, as deff_flux sums it on such a context."""
    nx, ny, B = 40, 32, 3
    imgs = masks(oracle, nx, ny, 7)
    with onchip(pkg, nx, ny, nimg=B) as s:
        s.set_tuning("flux_reduce", 2)
        res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, want_fields=True)
        d, _, _ = s.flux()
        held = {r.slot: r for r in res}                               # the later image of a slot stays
        assert sorted(held) == [0, 1, 2]
        for k in range(B):
            assert held[k].deff_raw == d[k], (k, held[k].deff_raw, d[k])
    for pix, r in zip(imgs, res):                                     # everything but the sum's order is the one-image call's
        want, x, _, _ = one_image(pkg, pix)
        assert (r.iters, r.rel_residual, r.converged) == (want[0], want[1], want[3]) and np.array_equal(r.field, x)
        # a tree against a serial sum of each wall's 32 fluxes, all of one sign: each sum is within 31 eps of the exact one
        assert abs(r.deff_raw - want[2]) <= 64 * np.finfo(np.float64).eps * abs(want[2])


def test_df_zero_is_admitted_as_by_solve_cg(pkg, oracle):
    """Df = 0 is no refusal: the fluid's rows are decoupled (four zero links, b = 0), which cg_table skips, exactly as
    deff_solve_cg takes such a system; the stream gives that call's bits, and x = 0 on the fluid."""
    nx, ny = 40, 32
    imgs = masks(oracle, nx, ny, 5)
    with onchip(pkg, nx, ny, nimg=2) as s:
        res = s.solve_cg_stream(imgs, 1e-3, 0.0, 0.0, 1.0, want_fields=True)
        assert s.plan_value("cg_impl") == 2
    for pix, r in zip(imgs, res):
        with onchip(pkg, nx, ny) as s1:
            s1.set_image(pix)
            s1.assemble_2phase(1e-3, 0.0, 0.0, 1.0)
            s1.init_linear(0.0, 1.0)
            r1 = s1.solve_cg(rtol=1e-10)
            assert bits(r) == bits(r1) and np.array_equal(r.field, s1.get_field())
        assert np.all(np.isfinite(r.field)) and np.all(r.field[pix < 150] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. Stop paths and refusals

def test_max_iter_zero_drains_the_source(pkg, oracle):
    imgs = masks(oracle, 40, 32, 8)
    res, impl, _ = run_stream(pkg, imgs, 3, max_iter=0)
    assert len(res) == 8 and impl == 2
    x0 = oracle.linear_guess(40, 32, 0.0, 1.0)
    for pix, r in zip(imgs, res):
        assert r.iters == 0 and not r.converged and np.array_equal(r.field, x0)
    assert_one_image_bits(pkg, imgs, res, 2, max_iter=0)


def test_rtol_zero_stops_at_max_iter(pkg, oracle):
    imgs = masks(oracle, 40, 32, 5)
    res, _, _ = run_stream(pkg, imgs, 3, rtol=0.0, max_iter=50, ce=7)
    assert [r.iters for r in res] == [50] * 5 and not any(r.converged for r in res)
    assert_one_image_bits(pkg, imgs, res, 2, rtol=0.0, max_iter=50)


def test_fewer_images_than_slots_and_none(pkg, oracle):
    imgs = masks(oracle, 33, 21, 2)
    with onchip(pkg, 33, 21, nimg=4) as s:
        res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, want_fields=True)
        assert_one_image_bits(pkg, imgs, res, 2)
        assert sorted(r.slot for r in res) == [0, 1]
        X = s.get_field()
        for r in res:
            assert np.array_equal(X[r.slot * 21:(r.slot + 1) * 21], r.field)
        assert not X[2 * 21:].any()                                   # the slots that never received an image read 0
        assert s.solve_cg_stream([], 1e-3, 1.0, 0.0, 1.0) == []       # no image at all
        assert not s.get_field().any()
        assert [r.iters for r in s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0)] == [r.iters for r in res]


def test_source_error_leaves_a_usable_context(pkg, oracle):
    imgs = masks(oracle, 40, 32, 5)

    def failing():
        yield imgs[0]
        yield imgs[1]
        raise RuntimeError("third image")

    with onchip(pkg, 40, 32, nimg=2) as s:
        with pytest.raises(RuntimeError, match="third image"):
            s.solve_cg_stream(failing(), 1e-3, 1.0, 0.0, 1.0)
        # the C ABI's answer to a `next` that returns -1
        L, cap = pkg._capi.load(), pkg._capi
        calls = [0]

        def nxt(_u, _slot, pix_ptr, id_ptr):
            calls[0] += 1
            if calls[0] == 3:
                return -1
            C.memmove(pix_ptr, imgs[calls[0]].ctypes.data, imgs[0].size)
            id_ptr[0] = calls[0]
            return 1

        rc = L.deff_solve_cg_stream(s._ctx, 40, 32, 1, 1, 1e-3, 1.0, 0.0, 1.0, 1e-10, 100000, 64, cap.NEXT_IMAGE_FN(nxt),
                                    cap.CG_IMAGE_DONE_FN(lambda *a: None), None)
        assert rc == -1 and calls[0] == 3
        res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, want_fields=True)
        assert_one_image_bits(pkg, imgs, res, 2)


def test_refusals_come_before_the_first_image(pkg, oracle):
    L, cap = pkg._capi.load(), pkg._capi
    calls = [0]

    def nxt(*a):
        calls[0] += 1
        return 0

    fn, dn = cap.NEXT_IMAGE_FN(nxt), cap.CG_IMAGE_DONE_FN(lambda *a: None)
    null_next, null_done = C.cast(None, cap.NEXT_IMAGE_FN), C.cast(None, cap.CG_IMAGE_DONE_FN)

    def call(ctx, rtol=1e-10, max_iter=100, ce=64, Df=1.0, f=fn, d=dn, W=40, H=32):
        return L.deff_solve_cg_stream(ctx, W, H, 1, 1, 1e-3, Df, 0.0, 1.0, rtol, max_iter, ce, f, d, None)

    with onchip(pkg, 40, 32, nimg=2) as s:
        s.synth_image(SEED, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(3)
        x0 = s.get_field()
        assert call(s._ctx, f=null_next) == -1 and call(s._ctx, d=null_done) == -1
        for kw in (dict(rtol=-1e-10), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iter=-1), dict(ce=0),
                   dict(Df=-1.0), dict(Df=float("nan")), dict(W=41)):
            assert call(s._ctx, **kw) == -1, kw
        assert calls[0] == 0
        assert np.array_equal(s.get_field(), x0)                      # ... and nothing was touched
        s.sweeps(3)                                                   # the system is still the one assembled above
        D = oracle.fill_D_2phase(oracle.synth_mask(40, 32, SEED, 0), 1.0, 1e-3)
        A, b = oracle.discretize(D, 0.0, 1.0)
        assert np.array_equal(s.get_field()[:32], oracle.sweeps(A, b, oracle.linear_guess(40, 32, 0.0, 1.0), 6))
    with pkg.SlabRank(40, 32, 0, 1, transport=object()) as sr:       # one rank: the transport is never asked for anything
        assert call(sr._ctx) == -1 and b"slab" in L.deff_last_error()
    assert calls[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. What the context holds afterwards

def stream_into(s, imgs, **kw):
    res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, want_fields=True, **kw)
    held = {}
    for i, r in enumerate(res):
        held[r.slot] = i                                              # images of a slot run one after the other: the later one stays
    return res, held


def test_context_after_the_stream(pkg, oracle):
    nx, ny, B = 33, 21, 4
    imgs = masks(oracle, nx, ny, 7)
    with onchip(pkg, nx, ny, nimg=B) as s:
        res, held = stream_into(s, imgs)
        assert sorted(held) == list(range(B))
        X = s.get_field()
        d, _, _ = s.flux()
        for k in range(B):
            assert np.array_equal(X[k * ny:(k + 1) * ny], res[held[k]].field), k
            assert d[k] == res[held[k]].deff_raw, k
        # a CG call finds every slot converged: no iteration, the same numbers
        rc = s.solve_cg(rtol=1e-10)
        assert [r.iters for r in rc] == [0] * B and all(r.converged for r in rc)
        assert [(r.rel_residual, r.deff_raw) for r in rc] == [(res[held[k]].rel_residual, res[held[k]].deff_raw) for k in range(B)]
        assert np.array_equal(s.get_field(), X)
        # 27 Jacobi sweeps from there: the oracle's, slot by slot
        s.sweeps(27)
        got = s.get_field()
        for k in range(B):
            D = oracle.fill_D_2phase(imgs[held[k]], 1.0, 1e-3)
            A, b = oracle.discretize(D, 0.0, 1.0)
            assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(A, b, np.array(res[held[k]].field), 27)), k
        # a Jacobi stream on the same context: what a fresh context gives
        again = s.solve_stream(imgs[:5], 1e-3, 1.0, 0.0, 1.0, 1e-6, 57, check_every=10, want_fields=True)
    with pkg.Solver(nx, ny, nimg=B) as f:
        fresh = f.solve_stream(imgs[:5], 1e-3, 1.0, 0.0, 1.0, 1e-6, 57, check_every=10, want_fields=True)
    for a, b in zip(again, fresh):
        assert (a.iters, a.deff_raw, a.conv, a.slot) == (b.iters, b.deff_raw, b.conv, b.slot)
        assert np.array_equal(a.field, b.field)
    # empty slots, and a new image / assembly / guess on the used context
    with onchip(pkg, nx, ny, nimg=B) as s:
        res, held = stream_into(s, imgs[:2])
        X = s.get_field()
        for k in range(B):
            assert np.array_equal(X[k * ny:(k + 1) * ny], res[held[k]].field) if k in held else not X[k * ny:(k + 1) * ny].any()
        d, MFL, MFR = s.flux()
        assert np.all(np.isfinite(d)) and d[2] == 0.0 and d[3] == 0.0
        s.set_image(np.stack(imgs[3:7]))
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        rs = s.solve_cg(rtol=1e-10)
        for k in range(B):
            assert bits(rs[k]) == one_image(pkg, imgs[3 + k])[0], k


def test_slot_readers_inside_done(pkg, oracle):
    """deff_get_slot_field and deff_residual_slot for the reported slot, from inside the callback, while other slots run."""
    nx, ny = 40, 32
    imgs = masks(oracle, nx, ny, 6)
    L, cap = pkg._capi.load(), pkg._capi
    it = iter(enumerate(imgs))
    seen = {}

    def nxt(_u, _slot, pix_ptr, id_ptr):
        try:
            k, pix = next(it)
        except StopIteration:
            return 0
        C.memmove(pix_ptr, pix.ctypes.data, pix.size)
        id_ptr[0] = k
        return 1

    with onchip(pkg, nx, ny, nimg=2) as s:
        def dn(_u, image_id, slot, res_ptr):
            x = np.empty((ny, nx))
            r = C.c_double(-1.0)
            rc1 = L.deff_get_slot_field(s._ctx, slot, x)
            rc2 = L.deff_residual_slot(s._ctx, slot, C.byref(r))
            seen[int(image_id)] = (rc1, rc2, x, r.value, res_ptr[0].iters)

        rc = L.deff_solve_cg_stream(s._ctx, nx, ny, 1, 1, 1e-3, 1.0, 0.0, 1.0, 1e-10, 100000, 64, cap.NEXT_IMAGE_FN(nxt),
                                    cap.CG_IMAGE_DONE_FN(dn), None)
        assert rc == 0 and sorted(seen) == list(range(6))
    for k, pix in enumerate(imgs):
        rc1, rc2, x, r, iters = seen[k]
        want, xw, _, _ = one_image(pkg, pix)
        assert rc1 == 0 and rc2 == 0 and iters == want[0]
        assert np.array_equal(x, xw)
        oracle.assert_residual(r, x, oracle.fill_D_2phase(pix, 1.0, 1e-3), 0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Timing and the launch budget

def test_loop_ms_grows_along_the_stream(pkg, oracle):
    imgs = masks(oracle, 40, 32, 24)
    order = []
    with onchip(pkg, 40, 32, nimg=4) as s:
        L, cap = pkg._capi.load(), pkg._capi
        it = iter(enumerate(imgs))

        def nxt(_u, _slot, pix_ptr, id_ptr):
            try:
                k, pix = next(it)
            except StopIteration:
                return 0
            C.memmove(pix_ptr, pix.ctypes.data, pix.size)
            id_ptr[0] = k
            return 1

        def dn(_u, image_id, slot, res_ptr):
            order.append(res_ptr[0].loop_ms)

        t0 = time.perf_counter()
        rc = L.deff_solve_cg_stream(s._ctx, 40, 32, 1, 1, 1e-3, 1.0, 0.0, 1.0, 1e-10, 100000, 16, cap.NEXT_IMAGE_FN(nxt),
                                    cap.CG_IMAGE_DONE_FN(dn), None)
        wall_ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0 and len(order) == 24
    print(f"loop_ms {order[0]:.3f} ... {order[-1]:.3f}, wall {wall_ms:.3f} ms")
    assert all(a <= b for a, b in zip(order, order[1:])), order
    assert 0.0 < order[0] and order[-1] <= wall_ms


@pytest.mark.parametrize("B", [4, 32])
def test_launch_budget(pkg, oracle, B):
    """Launches and host waits per interval do not grow with the slots that retire or enter in it: on chip an interval is at
    most 1 (iteration) + 2 (true residual) + 1 (flux) + 1 (entry) + 1 (admissibility) + 2 (entry residual and check) = 8
    launches and 2 waits, plus a constant per call; the bound asserted is the issue's, 12 per interval + 16."""
    imgs = masks(oracle, 40, 32, 64)
    with onchip(pkg, 40, 32, nimg=B) as s:
        res = s.solve_cg_stream(imgs, 1e-3, 1.0, 0.0, 1.0, check_every=16)
        n, launches, waits = (s.plan_value(k) for k in ("cgs_intervals", "cgs_launches", "cgs_waits"))
    print(f"B={B}: {n} intervals, {launches} launches, {waits} waits")
    assert len(res) == 64 and all(r.converged for r in res)
    assert n >= max(r.iters for r in res) // 16
    assert 0 < launches <= 12 * n + 16 and 0 < waits <= 2 * n + 8


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Driver

def test_deff2d_cg_stream(tmp_path):
    """The 20 JPEGs of test_gpu_cg_onchip.py::test_deff2d_cg_batch (128 x 128 with a 64 x 64 and a 160 x 160 one in the
    middle), three ways: one image at a time, --cg-batch 8 and --cg-stream 8.
    Against --cg-batch 8 every number of every row is EQUAL except Time: both run k_cg_image for the 128 x 128 and 64 x 64
    images and the streaming kernels for the 160 x 160 one, and the library gives an image the bits of a one-image solve in
    a stack as in a stream -- Deff, iterations, stage_iterations, converge and the residual that cg_stream_done reads from the
    image's slot included.
    Against the one-image run, which iterates with the streaming kernels (the driver never sets "cg_onchip" there) while the
    stream runs on chip: the image columns are equal, Deff within 2 DEFF_TOL -- each run is within DEFF_TOL of the exact value
    at this rtol (test_gpu_cg.py), the bound test_deff2d_cg_batch uses for the same pair of forms."""
    from PIL import Image
    from test_frontend import _write_input
    rng = np.random.default_rng(20)
    sizes = [128] * 20
    sizes[9], sizes[10] = 64, 160
    for k, n in enumerate(sizes):
        a = rng.random((n // 8, n // 8)) < 0.35
        Image.fromarray(np.kron(np.where(a, 255, 0), np.ones((8, 8))).astype(np.uint8), "L").save(tmp_path / f"{k:05d}.jpg", quality=95)
    _write_input(tmp_path / "input.txt", Phases=2, Ds="1e-3", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0, OutputName="out.csv",
                 printCMap=0, Convergence="1e-6", MaxIter="5e5", Verbose=0, RunBatch=1, NumImages=20)
    runs = []
    for extra in ([], ["--cg-batch", "8"], ["--cg-stream", "8"]):
        out = f"res{len(runs)}.json"
        r = subprocess.run([EXE, "input.txt", "--json", out, "--solver", "cg", "--cg-rtol", "1e-13"] + extra, cwd=tmp_path,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        runs.append(json.load(open(tmp_path / out))["results"])
    plain, batched, streamed = runs
    assert len(plain) == 20 and len(batched) == 20 and len(streamed) == 20
    for a, b in zip(batched, streamed):
        assert set(a) == set(b) and {"Deff", "converge", "residual", "iterations", "stage_iterations", "Time"} <= set(a)
        for key in a:
            if key != "Time":
                assert a[key] == b[key], (key, a, b)
        assert b["iterations"] > 0 and b["stage_iterations"] == [b["iterations"]] and b["converge"] <= 1e-13, b
        assert b["residual"] is not None and b["Time"] > 0, b
    for a, b in zip(plain, streamed):
        for key in a:
            if key not in ("Deff", "converge", "residual", "iterations", "stage_iterations", "Time"):
                assert a[key] == b[key], (key, a, b)
        assert a["converge"] <= 1e-13 and a["iterations"] > 0, a
        assert abs(a["Deff"] - b["Deff"]) <= 2 * DEFF_TOL * abs(a["Deff"]), (a, b)
    rows = open(tmp_path / "out.csv").read().splitlines()
    assert len(rows) == 3 * 21                                       # the CSV is appended to: header + 20 rows per run
