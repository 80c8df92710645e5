"""The tuning key "cg_onchip_planes" on the GPU (kernels_cg_image_planes.hpp: one workgroup iterates one image of at most 16 384
cells on a compute unit, the matrix rows read from the coefficient planes): which form a call takes, the bits of the table
on-chip form wherever a dictionary exists, the fixed point of systems that have none, stacks, stop paths, the three side
solves (deff_solve_adjoint / _tangent / _adjoint_tangent), alternation with the other forms on one context, and the torch ops.

Where a result is compared at a tolerance the bar is test_gpu_cg_planes.py's rule max(1e-10, 10 d_ref), and d_ref is measured in
the test on the streaming plane form (key 0: the code path of every earlier revision), never on the kernel under test."""
import functools

import numpy as np
import pytest

from test_cg_host import RESTART_CASE, block_thomas, decoupled_of, rel_l2, residual_np
from test_gpu_cg import RTOL_PARITY, assert_fluxes_of_field, assert_honest, wall_clusters
from test_gpu_cg_onchip import SHAPES
from test_gpu_cg_planes import CELL_SYSTEMS, as_list, bits, dictionary_system, per_cell_system

pytestmark = pytest.mark.gpu

KEY = "cg_onchip_planes"


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def bar(d_ref):
    return max(1e-10, 10.0 * d_ref)


def solve(s, x0, **kw):
    """One solve_cg from x0: (bits, wall fluxes, field, cg_impl, cg_fold, cg_restarts)."""
    s.set_field(x0)
    r = s.solve_cg(**kw)
    assert_fluxes_of_field(s, r)
    flux = [(q.MFL.copy(), q.MFR.copy()) for q in as_list(r)]
    return bits(r), flux, s.get_field(), s.plan_value("cg_impl"), s.plan_value("cg_fold"), s.plan_value("cg_restarts")


def same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for (l0, r0), (l1, r1) in zip(a[1], b[1]):
        assert np.array_equal(l0, l1) and np.array_equal(r0, r1)
    assert np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Selection

def cell_D(nx, ny, seed, nimg=1):
    return np.random.default_rng(seed).uniform(0.5, 2.0, (nimg * ny, nx))


def test_selection_by_key_and_size(pkg, oracle):
    nx, ny = 128, 128
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(cell_D(nx, ny, 1), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        got = []
        for key, impl in ((0, 3), (1, 4), (0, 3)):
            s.set_tuning(KEY, key)
            t = solve(s, x0, rtol=1e-10)
            assert t[3] == impl and s.plan()["cg_impl"] == impl, (key, t[3])
            assert t[0][0][2] and t[0][0][0] > 0
            if impl == 4:
                assert t[4] == 0
            got.append(t)
        same(got[0], got[2])
        # a refused value changes neither the key nor the field
        s.set_tuning(KEY, 1)
        s.set_field(x0)
        for bad in (2, -1):
            with pytest.raises(pkg.DeffError) as ei:
                s.set_tuning(KEY, bad)
            assert ei.value.code == -1
            assert np.array_equal(s.get_field(), x0)
        t = solve(s, x0, rtol=1e-10)
        assert t[3] == 4
        same(t, got[1])
    # 130 x 128 = 16 640 cells: not eligible, the key changes nothing
    nx = 130
    got = []
    for key in (1, 0):
        with pkg.Solver(nx, ny) as s:
            s.set_tuning("cg_planes", 1)
            s.set_tuning(KEY, key)
            s.assemble_from_D(cell_D(nx, ny, 2), 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            t = solve(s, s.get_field(), rtol=1e-10)
            assert t[3] == 3 and t[0][0][2]
            got.append(t)
    same(got[0], got[1])
    # a system that has a dictionary keeps the table forms under cg_planes 1, whatever the key
    s, x0 = dictionary_system(pkg, oracle, "native", 40, 32)
    with s:
        s.set_tuning("cg_planes", 1)
        ref = {}
        for onchip in (0, 1):
            for key in (0, 1):
                s.set_tuning("cg_onchip", onchip)
                s.set_tuning(KEY, key)
                t = solve(s, x0, rtol=1e-10)
                assert t[3] == 1 + onchip, (onchip, key, t[3])
                same(ref.setdefault(onchip, t), t)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. Bits of the table on-chip form

def table_and_planes_agree(s, x0, **kw):
    s.set_tuning("cg_planes", 0)
    s.set_tuning("cg_onchip", 1)
    t = solve(s, x0, **kw)
    s.set_tuning("cg_planes", 2)
    s.set_tuning(KEY, 1)
    p = solve(s, x0, **kw)
    assert (t[3], p[3]) == (2, 4), (t[3], p[3])
    assert (t[4], p[4]) == (0, 0)
    same(t, p)
    assert t[5] == p[5], (t[5], p[5])
    return t


def check_bits_of_table_onchip(s, x0):
    for k in (1, 2, 3, 20):
        table_and_planes_agree(s, x0, rtol=0.0, max_iter=k)
    return table_and_planes_agree(s, x0, rtol=1e-10, max_iter=200000)


@pytest.mark.parametrize("nx,ny", SHAPES, ids=[f"{nx}x{ny}" for nx, ny in SHAPES])
def test_bits_of_the_table_onchip_form_native(pkg, oracle, nx, ny):
    s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
    with s:
        t = check_bits_of_table_onchip(s, x0)
        assert t[0][0][0] > 0


@pytest.mark.parametrize("name", ["from_D-4-levels", "sources-inside", "3phase-grid"])
def test_bits_of_the_table_onchip_form_systems(pkg, oracle, name):
    for nx, ny in ((130, 71), (97, 41)):
        s, x0 = dictionary_system(pkg, oracle, name, nx, ny)
        with s:
            check_bits_of_table_onchip(s, x0)


def test_bits_of_the_table_onchip_form_shipped_options(pkg, img00000):
    """The shipped 3-phase options (Grid / ImpSolid rows: decoupled cells inside the image), Ds = 0, and a two-valued D map."""
    ny, nx = img00000.shape
    grid, _ = pkg.flood_fill((img00000 > 200).astype(np.uint32))
    with pkg.Solver(nx, ny) as s:
        s.set_image(img00000)
        s.assemble_3phase(0.0, 1.0, 1237500.0, 0.0, 1.0, grid)
        s.init_linear(0.0, 1.0)
        A, b = s.get_system()
        assert decoupled_of(A, b).sum() > 0
        check_bits_of_table_onchip(s, s.get_field())
    with pkg.Solver(nx, ny) as s:
        s.set_image(img00000)
        s.assemble_2phase(0.0, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        check_bits_of_table_onchip(s, s.get_field())
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(np.where(img00000 < 150, 1.0, 1e-2), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        check_bits_of_table_onchip(s, s.get_field())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. Systems without a dictionary

@pytest.mark.parametrize("case", CELL_SYSTEMS)
def test_fixed_point_of_systems_without_a_dictionary(pkg, oracle, case):
    """Key 1 against the direct solve; the bar is max(1e-10, 10 d_ref) with d_ref the distance the streaming plane form (key 0)
    leaves on the same case at the same rtol -- for the field (rel-L2) and for Deff (against deff_flux of the exact field)."""
    s, nx, ny, D, CL, CR = per_cell_system(pkg, oracle, case)
    with s:
        s.set_tuning("cg_planes", 1)
        x0 = s.get_field()
        A, b = s.get_system()
        dec = decoupled_of(A, b)
        fixed, sel = dec, ~dec
        if case.startswith("grid"):
            wall, isolated = wall_clusters(A, b, nx, ny)
            fixed, sel = dec | isolated, wall
        xd = block_thomas(A, b, nx, ny, fixed)
        s.set_field(xd)
        d_exact = s.flux()[0]
        out = {}
        for key in (0, 1):
            s.set_tuning(KEY, key)
            t = solve(s, x0, rtol=RTOL_PARITY)
            r = s.solve_cg(rtol=RTOL_PARITY)                         # from the converged field: 0 iterations, the same result
            assert t[3] == 3 + key and t[0][0][2] and t[0][0][0] > 0, (key, t[0])
            assert r.iters == 0 and r.converged and np.array_equal(s.get_field(), t[2])
            assert_honest(r, RTOL_PARITY, A, b, t[2], nx, ny)
            assert np.all(t[2].ravel()[dec] == 0.0) and np.all(np.isfinite(t[2]))
            out[key] = (rel_l2(t[2].ravel()[sel], xd.ravel()[sel]), abs(t[0][0][3] - d_exact) / abs(d_exact), t[0][0][0])
        (d_ref, deff_ref, it0), (d, deff, it1) = out[0], out[1]
        print(f"{case}: streaming planes {it0} iterations field {d_ref:.3e} Deff {deff_ref:.3e}; on chip {it1} iterations "
              f"field {d:.3e} Deff {deff:.3e}")
        assert d <= bar(d_ref), (d, d_ref)
        assert deff <= bar(deff_ref), (deff, deff_ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Stacks

def stack_D(n, B):
    """A distinct seeded D per image; the contrast grows with the image's number modulo 4, so the iteration counts differ."""
    rng = np.random.default_rng(96)
    return [10.0 ** rng.uniform(-0.5 * (1 + k % 4), 0.0, (n, n)) for k in range(B)]


def stack_run(pkg, Ds, n, check_every):
    B = len(Ds)
    with pkg.Solver(n, n, nimg=B) as s:
        s.set_tuning("cg_planes", 1)
        s.set_tuning(KEY, 1)
        s.assemble_from_D(np.concatenate(Ds), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        rs = s.solve_cg(rtol=1e-10, check_every=check_every)
        assert s.plan_value("cg_impl") == 4
        assert_fluxes_of_field(s, rs)
        return bits(rs), s.get_field()


@pytest.mark.parametrize("B", [3, 300])
def test_stack_gives_the_bits_of_single_images(pkg, B):
    """300 images are more than the chip has compute units: workgroups take several.  Every image gives the bits of a
    one-image context, whatever check_every (the state is saved and reloaded between launches)."""
    n = 96
    Ds = stack_D(n, B)
    rs0, X0 = stack_run(pkg, Ds, n, 64)
    assert all(r[2] for r in rs0) and len({r[0] for r in rs0}) > 1
    for ce in (1, 7, 1000):
        rs, X = stack_run(pkg, Ds, n, ce)
        assert rs == rs0, ce
        assert np.array_equal(X, X0), ce
    with pkg.Solver(n, n) as s1:
        s1.set_tuning("cg_planes", 1)
        s1.set_tuning(KEY, 1)
        for k in range(B):
            s1.assemble_from_D(Ds[k], 0.0, 1.0)
            s1.init_linear(0.0, 1.0)
            r1 = s1.solve_cg(rtol=1e-10)
            assert s1.plan_value("cg_impl") == 4
            assert bits(r1)[0] == rs0[k], (k, r1, rs0[k])
            assert np.array_equal(s1.get_field(), X0[k * n:(k + 1) * n]), k


def test_stack_with_an_image_done_at_the_start(pkg):
    """Image 1 of 3 has a uniform D and starts from its exact solution: frozen before the first iteration, no writes."""
    nx, ny = 33, 20
    rng = np.random.default_rng(3)
    Ds = [rng.uniform(0.5, 2.0, (ny, nx)), np.ones((ny, nx)), rng.uniform(0.5, 2.0, (ny, nx))]
    ramp = np.tile((np.arange(nx) + 0.5) / nx, (ny, 1))
    with pkg.Solver(nx, ny, nimg=3) as s:
        s.set_tuning("cg_planes", 2)
        s.set_tuning(KEY, 1)
        s.assemble_from_D(np.concatenate(Ds), 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        X0 = s.get_field()
        X0[ny:2 * ny] = ramp
        s.set_field(X0)
        rs = s.solve_cg(rtol=1e-12)
        X = s.get_field()
        assert s.plan_value("cg_impl") == 4
        assert_fluxes_of_field(s, rs)
    assert rs[1].iters == 0 and rs[1].converged and rs[0].iters > 0 and rs[2].iters > 0
    assert np.array_equal(X[ny:2 * ny], X0[ny:2 * ny])
    for k in (0, 2):
        with pkg.Solver(nx, ny) as s1:
            s1.set_tuning("cg_planes", 2)
            s1.set_tuning(KEY, 1)
            s1.assemble_from_D(Ds[k], 0.0, 1.0)
            s1.init_linear(0.0, 1.0)
            r1 = s1.solve_cg(rtol=1e-12)
            assert s1.plan_value("cg_impl") == 4 and r1.converged and rs[k].converged
            assert bits(r1) == bits(rs[k])
            assert np.array_equal(X[k * ny:(k + 1) * ny], s1.get_field()), k


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Stop paths, against key 0's verdicts

def test_stop_paths(pkg, oracle):
    nx, ny = 40, 32
    rng = np.random.default_rng(5)
    D = rng.uniform(0.5, 2.0, (ny, nx))
    D[8:16, 10:20] = 0.0
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        A, b = s.get_system()
        dec = decoupled_of(A, b).reshape(ny, nx)
        assert dec.sum() == 80
        for kw in (dict(rtol=1e-10, max_iter=0), dict(rtol=1e-10, max_iter=3), dict(rtol=0.0, max_iter=50, check_every=7)):
            got = {}
            for key in (0, 1):
                s.set_tuning(KEY, key)
                t = solve(s, x0, **kw)
                assert t[3] == 3 + key and t[5] == 0
                (iters, rel, conv, _), = t[0]
                assert iters == kw["max_iter"] and not conv
                res = residual_np(A, b, t[2], nx, ny)
                assert abs(rel - res) <= 1e-9 * res, (rel, res)
                assert np.all(t[2][dec] == 0.0) and np.all(np.isfinite(t[2]))
                got[key] = t
            if kw["max_iter"] == 0:
                same(got[0], got[1])                                 # no iteration ran: the start is the streaming form's
                assert np.array_equal(got[1][2][~dec], x0[~dec])
    # b = 0 with x = 0: converged at once, 0 iterations, residual 0
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, 0.0, 0.0)
        assert np.all(s.get_system()[1] == 0.0)
        for key in (0, 1):
            s.set_tuning(KEY, key)
            s.set_field(np.zeros((ny, nx)))
            r = s.solve_cg(rtol=1e-10)
            assert s.plan_value("cg_impl") == 3 + key
            assert r.converged and r.rel_residual == 0.0 and r.iters == 0 and np.all(s.get_field() == 0.0)
            assert_fluxes_of_field(s, r)


def test_restart_round(pkg, oracle):
    """test_gpu_cg_planes.py::test_planes_restart_round's construction: the recurrence's residual meets an rtol that the true
    residual misses, so a true-residual round sends the image back.  The same verdicts as key 0 and the bits of the table
    on-chip form."""
    nx, ny, Ds, rtol = RESTART_CASE
    with pkg.Solver(nx, ny) as s:
        s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
        s.assemble_2phase(Ds, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        A, b = s.get_system()
        t = table_and_planes_agree(s, x0, rtol=rtol)
        assert t[5] >= 1, t[5]
        s.set_tuning(KEY, 0)
        p0 = solve(s, x0, rtol=rtol)
        assert p0[3] == 3 and p0[5] >= 1
        assert t[0][0][2] and p0[0][0][2]
        assert residual_np(A, b, t[2], nx, ny) <= 2 * rtol


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Side solves

SIDE_CASES = [(1, 40, 32), (1, 130, 71), (3, 33, 20)]


@functools.lru_cache(maxsize=None)
def side_case(nimg, nx, ny):
    rng = np.random.default_rng(1000 * nimg + nx + ny)
    D = np.exp(rng.standard_normal((nimg * ny, nx)))
    D[rng.random((nimg * ny, nx)) < 0.03] = 0.0
    D[3, 0] = 0.0
    w = rng.standard_normal((nimg * ny, nx))
    dD = rng.standard_normal((nimg * ny, nx)) * D
    for a in (D, w, dD):
        a.setflags(write=False)
    return D, w, dD


def direct(A, rhs, dec, nimg, nx, ny):
    """A y = rhs (zeroed on the decoupled cells) image by image, decoupled cells fixed at 0."""
    n = nx * ny
    rhs = np.where(dec, 0.0, rhs.ravel())
    return np.concatenate([block_thomas(A[k * n:(k + 1) * n], rhs[k * n:(k + 1) * n], nx, ny, fixed=dec[k * n:(k + 1) * n]).ravel()
                           for k in range(nimg)]).reshape(nimg * ny, nx)


def side_run(s, key, D, w, dD, CL, CR, rtol):
    """The three side solves and the four maps after them under `key`; checks what they must leave alone."""
    s.set_tuning(KEY, key)
    x = s.get_field()
    A, b = s.get_system()
    state = tuple(s.plan_value(k) for k in ("dict_outcome", "dict_rows", "lut_rows"))
    out = {}
    ra = as_list(s.solve_adjoint(w, rtol=rtol))
    assert s.plan_value("cg_impl") == 3 + key and s.plan_value("cg_fold") == 0
    out["lam"] = s.get_adjoint()
    out["vjp"] = np.asarray(s.field_vjp(D, CL, CR)[0]).reshape(-1, s.nx)
    out["r"] = np.asarray(s.tangent_rhs(D, dD, CL, CR)[0]).reshape(-1, s.nx)
    rt = as_list(s.solve_tangent(rtol=rtol))
    assert s.plan_value("cg_impl") == 3 + key
    out["dx"] = s.get_tangent()
    out["q"] = np.asarray(s.adjoint_tangent_rhs(D, dD)[0]).reshape(-1, s.nx)
    rq = as_list(s.solve_adjoint_tangent(rtol=rtol))
    assert s.plan_value("cg_impl") == 3 + key
    out["dl"] = s.get_adjoint_tangent()
    assert all(r.converged and r.iters > 0 and r.deff_raw == 0.0 for r in ra + rt + rq), (ra, rt, rq)
    out["jvp"] = s.field_jvp(D, dD, CL, CR, rtol=rtol)
    assert s.plan_value("cg_impl") == 3 + key
    out["deff_hvp"] = np.asarray(s.deff_hvp(D, dD, CL, CR, rtol=rtol)[0]).reshape(-1, s.nx)
    assert s.plan_value("cg_impl") == 3 + key
    out["field_hvp"] = np.asarray(s.field_hvp(D, dD, CL, CR, rtol=rtol)[0]).reshape(-1, s.nx)
    assert s.plan_value("cg_impl") == 3 + key
    A1, b1 = s.get_system()
    assert np.array_equal(s.get_field(), x) and np.array_equal(A1, A) and np.array_equal(b1, b)
    assert state == tuple(s.plan_value(k) for k in ("dict_outcome", "dict_rows", "lut_rows"))
    return out


@pytest.mark.parametrize("nimg,nx,ny", SIDE_CASES)
def test_side_solves(pkg, nimg, nx, ny):
    """lambda, dx and dlambda of key 1 against direct solves of the same systems (the right-hand sides are the library's own
    maps); d_ref is key 0's distance.  The maps that read them (field_vjp, field_jvp, deff_hvp, field_hvp) against their key-0
    values: they are linear in each solved field, so the bar is the rule's on the sum of key 0's distances of the fields read."""
    CL, CR, rtol = 2.0, -1.0, 1e-13
    D, w, dD = side_case(nimg, nx, ny)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_tuning("cg_planes", 1)
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        assert all(r.converged for r in as_list(s.solve_cg(rtol=rtol)))
        A, b = s.get_system()
        dec = decoupled_of(A, b)
        o0 = side_run(s, 0, D, w, dD, CL, CR, rtol)
        o1 = side_run(s, 1, D, w, dD, CL, CR, rtol)
    dref = {}
    for name, rhs in (("lam", "w"), ("dx", "r"), ("dl", "q")):
        if rhs == "r":
            assert np.array_equal(o0["r"], o1["r"])                  # a pass over (x, D, dD): no solve in it (q reads lambda)
        y0 = direct(A, w if rhs == "w" else o0[rhs], dec, nimg, nx, ny)
        y1 = direct(A, w if rhs == "w" else o1[rhs], dec, nimg, nx, ny)
        dref[name] = rel_l2(o0[name], y0)
        d = rel_l2(o1[name], y1)
        print(f"side solves {nimg} x {nx}x{ny} {name}: key 0 {dref[name]:.3e}  key 1 {d:.3e}")
        assert np.all(o1[name].ravel()[dec] == 0.0)
        assert d <= bar(dref[name]), (name, d, dref[name])
    reads = {"vjp": ("lam",), "jvp": ("dx",), "deff_hvp": ("dx",), "field_hvp": ("lam", "dx", "dl")}
    for name, fields in reads.items():
        d = rel_l2(o1[name], o0[name])
        ref = sum(dref[f] for f in fields)
        print(f"side solves {nimg} x {nx}x{ny} {name}: key 1 against key 0 {d:.3e}  (key 0's fields {ref:.3e})")
        assert d <= bar(ref), (name, d, ref)


@pytest.mark.parametrize("nimg,nx,ny", SIDE_CASES)
def test_adjoint_solve_equals_twin_forward_solve(pkg, nimg, nx, ny):
    """test_gpu_field_vjp.py's twin under key 1: context B holds A's matrix with w' (w zeroed where A's forward system decouples
    the cell, as k_cgp_mask_rhs does) as its right-hand side and solves it as a forward system (cg_planes 2, key 1) from x = 0:
    the bits of solve_adjoint(w) under key 1, for every check_every."""
    CL, CR = 2.0, -1.0
    D, w, _ = side_case(nimg, nx, ny)
    with pkg.Solver(nx, ny, nimg=nimg) as a, pkg.Solver(nx, ny, nimg=nimg) as b:
        a.assemble_from_D(D, CL, CR)
        Am, bm = a.get_system()
        dec = decoupled_of(Am, bm).reshape(nimg * ny, nx)
        assert dec.any()
        b.set_system(Am, np.where(dec, 0.0, w).ravel(), D, CL, CR)
        b.set_tuning("cg_planes", 2)
        b.set_tuning(KEY, 1)
        b.set_field(np.zeros((nimg * ny, nx)))
        rb = as_list(b.solve_cg(rtol=1e-11))
        xb = b.get_field()
        assert b.plan_value("cg_impl") == 4 and all(r.converged and r.iters > 10 for r in rb), rb
        a.set_tuning(KEY, 1)
        for every in (64, 1, 7):
            ra = as_list(a.solve_adjoint(w, rtol=1e-11, check_every=every))
            lam = a.get_adjoint()
            assert a.plan_value("cg_impl") == 4 and a.plan_value("cg_fold") == 0
            assert np.array_equal(lam, xb), every
            assert np.all(lam[dec] == 0.0)
            for k in range(nimg):
                assert (ra[k].iters, ra[k].rel_residual, ra[k].converged) == (rb[k].iters, rb[k].rel_residual, rb[k].converged)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. Alternation on one context

def test_key1_solve_does_not_leak_into_jacobi(pkg):
    nx, ny = 64, 48
    D = cell_D(nx, ny, 7)

    def jacobi(s, x0):
        s.set_field(x0)
        s.sweeps(5)
        x5 = s.get_field()
        s.set_field(x0)
        r = s.solve(1e-7, 2001, check_every=1000)
        return x5, (r.iters, r.deff_raw, r.conv), s.get_field()

    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        x0 = s.get_field()
        want = jacobi(s, x0)
    with pkg.Solver(nx, ny) as s:
        s.set_tuning("cg_planes", 1)
        s.set_tuning(KEY, 1)
        s.assemble_from_D(D, 0.0, 1.0)
        s.set_field(x0)
        r = s.solve_cg(rtol=1e-10)
        assert r.converged and s.plan_value("cg_impl") == 4
        got = jacobi(s, x0)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])


def test_forms_alternate_on_one_context(pkg, oracle):
    """cg_impl 2 -> 4 -> 3 -> 4 -> 1 -> 4 on one context (they share cg_p[0], the scalars and the restart flag): each solve
    gives the bits of a fresh context under the same keys, for a few iterations and to rtol."""
    nx, ny = 130, 71
    forms = {1: (0, 0, 0), 2: (0, 1, 0), 3: (2, 0, 0), 4: (2, 0, 1)}          # cg_impl: (cg_planes, cg_onchip, key)

    def setup(s, impl):
        for k, v in zip(("cg_planes", "cg_onchip", KEY), forms[impl]):
            s.set_tuning(k, v)

    for kw in (dict(rtol=0.0, max_iter=7), dict(rtol=1e-10)):
        fresh = {}
        for impl in forms:
            s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
            with s:
                setup(s, impl)
                fresh[impl] = solve(s, x0, **kw)
                assert fresh[impl][3] == impl
        same(fresh[2], fresh[4])
        same(fresh[1], fresh[3])
        s, x0 = dictionary_system(pkg, oracle, "native", nx, ny)
        with s:
            for impl in (2, 4, 3, 4, 1, 4):
                setup(s, impl)
                t = solve(s, x0, **kw)
                assert t[3] == impl
                same(t, fresh[impl])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. torch

@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("nimg", [1, 2])
def test_torch_ops(pkg, device, nimg):
    """onchip=True against onchip=False: value, gradient and one functional.hvp of effective_diffusivity and of a loss on
    concentration_field, at 12 x 9.  d_ref: what onchip=False itself moves between rtol 1e-12 (the default, used by both) and
    1e-13 -- the streaming form's own distance from a tighter answer; the bar is the rule's.  With onchip=False the ops give
    the bits of the Solver calls they are documented to make."""
    import torch
    from torch.autograd.functional import hvp
    ny, nx = 9, 12
    rng = np.random.default_rng(12 + nimg)
    shape = (nimg, ny, nx) if nimg > 1 else (ny, nx)
    Dh = rng.uniform(0.5, 2.0, shape)
    vh = rng.standard_normal(shape)
    ch = rng.standard_normal(shape)
    D = torch.tensor(Dh, device=device, requires_grad=True)
    v = torch.tensor(vh, device=device)
    c = torch.tensor(ch, device=device)

    def rel(a, b):
        a, b = a.detach().cpu().numpy().ravel(), b.detach().cpu().numpy().ravel()
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    def everything(**kw):
        deff = pkg.effective_diffusivity(D, **kw)
        g, = torch.autograd.grad(deff.sum(), D)
        _, h = hvp(lambda t: pkg.effective_diffusivity(t, **kw).sum(), D.detach(), v)
        loss = lambda t: (pkg.concentration_field(t, **kw) * c).sum() + 0.5 * (pkg.concentration_field(t, **kw) ** 2).sum()
        x = pkg.concentration_field(D, **kw)
        gx, = torch.autograd.grad(loss(D), D)
        _, hx = hvp(loss, D.detach(), v)
        return dict(deff=deff, g=g, h=h, x=x, gx=gx, hx=hx)

    off = everything()
    tight = everything(rtol=1e-13)
    on = everything(onchip=True)
    for name in off:
        d_ref, d = rel(off[name], tight[name]), rel(on[name], off[name])
        print(f"torch {device} nimg {nimg} {name}: onchip against not {d:.3e}  d_ref {d_ref:.3e}")
        assert on[name].device == D.device and on[name].shape == off[name].shape
        assert d <= bar(d_ref), (name, d, d_ref)
    # a passed solver: the key is set by onchip=True in every pass and the side solves take the on-chip form
    D2 = Dh.reshape(nimg * ny, nx)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        x = pkg.concentration_field(D, solver=s, onchip=True)
        (x * c).sum().backward()
        assert s.plan_value("cg_impl") == 4
        D.grad = None
    # onchip=False: today's calls, today's bits
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(D2, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.set_tuning("cg_planes", 1)
        rs = as_list(s.solve_cg(rtol=1e-12, max_iter=1_000_000))
        g, _ = s.sensitivity(D2, 0.0, 1.0)
        xs = s.get_field()
        assert s.plan_value("cg_impl") in (1, 3)
        assert np.array_equal(np.atleast_1d(off["deff"].detach().cpu().numpy()), np.array([r.deff_raw for r in rs]))
        assert np.array_equal(off["g"].cpu().numpy().reshape(-1, nx), np.asarray(g).reshape(-1, nx))
        assert np.array_equal(off["x"].detach().cpu().numpy().reshape(-1, nx), xs)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        xt = pkg.concentration_field(D, solver=s)
        (xt * c).sum().backward()
        got = D.grad.detach().cpu().numpy().reshape(-1, nx)
        D.grad = None
        assert s.plan_value("cg_impl") == 3
        s.assemble_from_D(D2, 0.0, 1.0)
        s.set_field(xs)
        assert all(r.converged for r in as_list(s.solve_adjoint(ch.reshape(nimg * ny, nx), rtol=1e-12, max_iter=1_000_000)))
        assert s.plan_value("cg_impl") == 3
        want, _ = s.field_vjp(D2, 0.0, 1.0)
        assert np.array_equal(got, np.asarray(want).reshape(-1, nx))
