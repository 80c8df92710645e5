"""The Deff Hessian-vector product on the GPU (deff_sensitivity_hvp_D, deff_set_tangent; csrc/kernels_facepass.hpp with
HvpPass): the pass bit for bit against the numpy model of the normative expressions at every strip / seam / pad shape on
arbitrary planes, the whole product against the model on direct solves, the identities that need no reference on the device
(H D = 0, symmetry, concavity), what the call leaves alone, refusals, and the second derivative of the torch op."""
import ctypes as C
import functools

import numpy as np
import pytest

from sens_hvp_model import sens_hvp as model
from tangent_model import tangent_rhs
from test_cg_host import block_thomas, decoupled_of, pcg_numpy, rel_l2
from test_gpu_sensitivity import _refused, device_rows, make_case

pytestmark = pytest.mark.gpu

WALLS = [(0.0, 1.0), (2.0, -1.0)]
CURV_BAR = 1e-13                                         # curv against the model's long-double sum, relative to it


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_planes(D, seed):
    """A random direction, non-zero on every cell -- the cells with D == 0 included, where the pass has to ignore it --, and a
    random plane for dx (the pass is a function of any four planes)."""
    rng = np.random.default_rng(seed + 277)
    dD = rng.standard_normal(D.shape)
    dD[dD == 0.0] = 1.0
    return dD, rng.standard_normal(D.shape)


# ---- the pass, bit for bit ----------------------------------------------------------------------------------------------

def check_map(pkg, nx, ny, nimg, CL, CR, kt=0, seed=0):
    """The map equals the model's (array_equal), curv is within 1e-13 relative of the model's long-double sum and the same bits
    on a second call; the field and the tangent are unchanged; the device map is the host map with a pad column of 0.  Returns
    (hvp_kt, hvp_items) as used."""
    x, D = make_case(nx, ny, nimg, CL, CR, seed)
    dD, y = make_planes(D, seed)
    out = [model(x[k], y[k], D[k], dD[k], CL, CR) for k in range(nimg)]
    want, cv_want = np.stack([h for h, _ in out]), [c for _, c in out]
    rows = nimg * ny
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(D.reshape(rows, nx), CL, CR)
        s.set_field(x.reshape(rows, nx))
        s.set_tangent(y.reshape(rows, nx))
        if kt:
            s.set_tuning("hvp_kt", kt)
        hv, cv = s.sens_hvp(D.reshape(rows, nx), dD.reshape(rows, nx), CL, CR)
        hv2, cv2 = s.sens_hvp(D.reshape(rows, nx), dD.reshape(rows, nx), CL, CR)
        plan = s.plan_value("hvp_kt"), s.plan_value("hvp_items")
        assert np.array_equal(s.get_field(), x.reshape(rows, nx))
        assert np.array_equal(s.get_tangent(), y.reshape(rows, nx))
        p, pitch = s.device_sens_hvp_ptr()
        dev = device_rows(p, rows, pitch)
        assert pitch == s.device_field_ptr()[1] == 8 * (nx + (nx & 1))
        assert np.array_equal(dev[:, :nx], hv.reshape(rows, nx)) and np.all(dev[:, nx:] == 0.0)
    hv, hv2 = hv.reshape(nimg, ny, nx), hv2.reshape(nimg, ny, nx)
    cv, cv2 = np.atleast_1d(cv), np.atleast_1d(cv2)
    for k in range(nimg):
        bad = np.argwhere(hv[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), hv[k][tuple(bad[0])], want[k][tuple(bad[0])])
        rel = abs(float(np.longdouble(cv[k]) - cv_want[k])) / abs(float(cv_want[k]))
        print(f"sens hvp {nimg} x {nx}x{ny} kt {plan[0]} image {k}: curv {cv[k]:.6e}, off the model's by {rel:.3e} of it")
        assert rel <= CURV_BAR, (k, cv[k], cv_want[k])
    assert np.array_equal(hv, hv2) and np.array_equal(cv, cv2)
    assert np.all(hv[D == 0.0] == 0.0) and np.any(hv != 0.0) and np.all(np.isfinite(hv))
    return plan


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 5), (127, 17), (129, 17), (130, 71), (258, 9), (1030, 37)])
def test_map_matches_model(pkg, nx, ny, CL, CR):
    kt, items = check_map(pkg, nx, ny, 1, CL, CR, seed=nx * 100 + ny)
    assert kt == 1 and items == ((nx + 127) // 128) * ((ny + 7) // 8)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nimg,nx,ny", [(3, 33, 20), (5, 130, 69)])
def test_map_matches_model_stacks(pkg, nimg, nx, ny, CL, CR):
    """Every image of a stack has its own first and last row."""
    check_map(pkg, nx, ny, nimg, CL, CR, seed=nimg)


@pytest.mark.parametrize("nimg,nx,ny", [(1, 130, 71), (5, 130, 69)])
@pytest.mark.parametrize("kt", [1, 2, 64])
def test_map_matches_model_at_work_item_seams(pkg, nimg, nx, ny, kt):
    """"hvp_kt": 9 tile rows, 2 strips -- kt = 1 has a seam every 8 rows (9 items per strip), kt = 2 every 16 (5 items, the last
    one 7 rows short), kt = 64 is clipped to the image (one item per strip, no seam)."""
    used, items = check_map(pkg, nx, ny, nimg, 0.0, 1.0, kt=kt, seed=7 + kt)
    assert (used, items) == {1: (1, 18), 2: (2, 10), 64: (9, 2)}[kt]


def test_map_matches_model_large(pkg):
    """2050 x 1537: 17 strips (the last one 2 columns wide), 193 tile rows, an odd height."""
    kt, items = check_map(pkg, 2050, 1537, 1, 0.0, 1.0, seed=99)
    assert items == 17 * ((193 + kt - 1) // kt)


# ---- the whole product against the direct solves, and the identities ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def direct_case(nx, ny):
    """One system per shape, shared and left unchanged: D = exp(2 N(0, 1)) with zero cells, two directions v and w; the model
    on the direct solves x = A^-1 b and dx = A^-1 r' (decoupled cells fixed at 0) for v; and what the model makes of numpy's
    float64 CG fields stopped at rtol 1e-13: its distance from that, its |H D| / |H v| and its miss of <w, H v> = <v, H w>.
    The reference's own error, which sets the bars."""
    import oracle_binding as ob
    ob.build()
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + ny + 1)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    D[rng.random((ny, nx)) < 0.03] = 0.0
    D[ny // 2, nx // 2 - 1:nx // 2 + 1] = 0.0
    D[3, 0] = 0.0
    v = D * rng.standard_normal((ny, nx)) + np.where(D == 0.0, 1.0, 0.0)
    w = D * rng.standard_normal((ny, nx)) + np.where(D == 0.0, -1.0, 0.0)
    A, b = ob.discretize(D, CL, CR)
    dec = decoupled_of(A, b).reshape(ny, nx)
    xd = block_thomas(A, b, nx, ny, fixed=dec.ravel())
    rp = np.where(dec, 0.0, tangent_rhs(xd, D, v, CL, CR)[0])
    yd = block_thomas(A, rp.ravel(), nx, ny, fixed=dec.ravel())
    hv_d, curv_d = model(xd, yd, D, v, CL, CR)
    # the same on numpy's CG fields
    zero = np.zeros((ny, nx))
    tx = pcg_numpy(A, b, ob.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-13).x

    def hvp_np(d):
        r = np.where(dec, 0.0, tangent_rhs(tx, D, d, CL, CR)[0])
        return model(tx, pcg_numpy(A, r.ravel(), zero, nx, ny, 50_000, np.float64, rtol=1e-13).x, D, d, CL, CR)[0]

    hv_np, hw_np, hD_np = hvp_np(v), hvp_np(w), hvp_np(D)
    dv, dw = np.where(D == 0.0, 0.0, v), np.where(D == 0.0, 0.0, w)
    lhs = float(np.sum(dw * hv_np))
    out = dict(CL=CL, CR=CR, D=D, v=v, w=w, dv=dv, dw=dw, hv_d=hv_d, curv_d=float(curv_d), d_ref=rel_l2(hv_np, hv_d),
               hD_np=float(np.max(np.abs(hD_np)) / np.max(np.abs(hv_np))),
               sym_np=abs(lhs - float(np.sum(dv * hw_np))) / abs(lhs))
    for q in out.values():
        if isinstance(q, np.ndarray):
            q.setflags(write=False)
    return out


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_hvp_end_to_end(pkg, nx, ny):
    """solve_cg(1e-13), then deff_hvp(rtol 1e-13) along v, w and D.  H v against the model on the direct solves: bar
    max(1e-10, 10 d_ref), d_ref the same distance when the model is fed numpy's float64 CG fields at that rtol.  |H D| / |H v|
    and the miss of <w, H v> = <v, H w>: within 10 x the same figures from numpy's CG fields, and at least 1e-9.  curv < 0."""
    c = direct_case(nx, ny)
    CL, CR, D = c["CL"], c["CR"], c["D"]
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        rx = s.solve_cg(rtol=1e-13)
        x = s.get_field()
        hv, cv = s.deff_hvp(D, c["v"], CL, CR, rtol=1e-13)
        hw, cw = s.deff_hvp(D, c["w"], CL, CR, rtol=1e-13)
        hD, cD = s.deff_hvp(D, D, CL, CR, rtol=1e-13)
        assert np.array_equal(s.get_field(), x)
    assert rx.converged
    d = rel_l2(hv, c["hv_d"])
    rel_D = float(np.max(np.abs(hD)) / np.max(np.abs(hv)))
    lhs, rhs = float(np.sum(c["dw"] * hv)), float(np.sum(c["dv"] * hw))
    sym = abs(lhs - rhs) / abs(lhs)
    print(f"sens hvp end to end {nx}x{ny}: d {d:.3e} (numpy CG {c['d_ref']:.3e}); |H D| / |H v| {rel_D:.3e} (numpy CG "
          f"{c['hD_np']:.3e}); <w, H v> {lhs:.9e} <v, H w> {rhs:.9e} rel {sym:.3e} (numpy CG {c['sym_np']:.3e}); curv {cv:.6e} "
          f"{cw:.6e} (direct {c['curv_d']:.6e})")
    assert d <= max(1e-10, 10 * c["d_ref"]), (d, c["d_ref"])
    assert rel_D <= max(1e-9, 10 * c["hD_np"]), (rel_D, c["hD_np"])
    assert sym <= max(1e-9, 10 * c["sym_np"]), (sym, c["sym_np"])
    assert cv < 0 and cw < 0
    assert np.all(hv[D == 0.0] == 0.0)


# ---- what the call leaves alone, refusals ----------------------------------------------------------------------------------

def test_call_leaves_everything_else_alone(pkg):
    """Field, system, lambda, dx, and the rhs, vjp and sensitivity maps are bitwise what they were."""
    nx, ny, nimg = 33, 20, 2                             # odd width: the device maps have a pad column
    CL, CR = 2.0, -1.0
    x, D = make_case(nx, ny, nimg, CL, CR, 21)
    dD, y = make_planes(D, 21)
    rows = nimg * ny
    x2, D2, dD2, y2 = (a.reshape(rows, nx) for a in (x, D, dD, y))
    lam = np.random.default_rng(4).standard_normal((rows, nx))
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.assemble_from_D(D2, CL, CR)
        s.set_field(x2)
        A0, b0 = s.get_system()
        s.set_adjoint(lam)
        s.set_tangent(y2)
        s.tangent_rhs(D2, dD2, CL, CR)
        s.field_vjp(D2, CL, CR)
        s.sensitivity(D2, CL, CR)
        ptrs = [s.device_tangent_rhs_ptr(), s.device_field_vjp_ptr(), s.device_sensitivity_ptr()]
        maps = [device_rows(p, rows, pitch) for p, pitch in ptrs]
        hv, _ = s.sens_hvp(D2, dD2, CL, CR)
        assert np.any(hv != 0.0)
        assert [s.device_tangent_rhs_ptr(), s.device_field_vjp_ptr(), s.device_sensitivity_ptr()] == ptrs
        for (p, pitch), m in zip(ptrs, maps):
            assert np.array_equal(device_rows(p, rows, pitch), m)
        assert np.array_equal(s.get_field(), x2) and np.array_equal(s.get_adjoint(), lam)
        assert np.array_equal(s.get_tangent(), y2)
        A1, b1 = s.get_system()
        assert np.array_equal(A1, A0) and np.array_equal(b1, b0)
        # the tangent a solve left serves as well as a caller's own, and the pass leaves it alone too
        assert all(r.converged for r in s.solve_tangent(rtol=1e-10))
        dx = s.get_tangent()
        h1, c1 = s.sens_hvp(D2, dD2, CL, CR)
        assert np.array_equal(s.get_tangent(), dx)
        s.set_tangent(dx)
        h2, c2 = s.sens_hvp(D2, dD2, CL, CR)
        assert np.array_equal(h1, h2) and np.array_equal(c1, c2)


def test_refusals_leave_the_map_alone(pkg, oracle):
    nx, ny = 33, 20                                      # odd width: the device map has a pad column
    CL, CR = 0.0, 1.0
    x, D = make_case(nx, ny, 1, CL, CR, 3)
    x, D = x[0], D[0]
    dD, y = make_planes(D, 3)
    L = pkg._capi.load()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)      # noqa: E731
    with pkg.Solver(nx, ny) as s:
        _refused(pkg, s.device_sens_hvp_ptr, -5)         # DEFF_ESTATE: no map yet
        _refused(pkg, lambda: s.set_tangent(y), -5, "no system")
        _refused(pkg, lambda: s.sens_hvp(D, dD, CL, CR), -5, "no field")
        s.set_field(x)
        _refused(pkg, lambda: s.sens_hvp(D, dD, CL, CR), -5, "tangent")
        s.assemble_from_D(D, CL, CR)
        s.set_field(x)
        _refused(pkg, lambda: s.sens_hvp(D, dD, CL, CR), -5, "tangent")    # a system, but before any solve or set_tangent
        s.tangent_rhs(D, dD, CL, CR)
        _refused(pkg, lambda: s.sens_hvp(D, dD, CL, CR), -5, "tangent")    # a right-hand side is no tangent
        _refused(pkg, s.device_sens_hvp_ptr, -5)
        s.set_tangent(y)
        hv0, cv0 = s.sens_hvp(D, dD, CL, CR)
        p, pitch = s.device_sens_hvp_ptr()
        dev = device_rows(p, ny, pitch)
        assert np.array_equal(dev[:, :nx], hv0) and np.all(dev[:, nx:] == 0.0)

        def unchanged():
            assert s.device_sens_hvp_ptr() == (p, pitch) and np.array_equal(device_rows(p, ny, pitch), dev)

        # NULL arguments, CR == CL
        assert L.deff_sensitivity_hvp_D(s._ctx, None, vp(dD), CL, CR, None, None, None) == -1 and b"D is NULL" in L.deff_last_error()
        assert L.deff_sensitivity_hvp_D(s._ctx, vp(D), None, CL, CR, None, None, None) == -1 and b"dD is NULL" in L.deff_last_error()
        assert L.deff_device_sensitivity_hvp(s._ctx, None, None) == -1
        assert L.deff_set_tangent(s._ctx, None) == -1
        unchanged()
        assert np.array_equal(s.get_tangent(), y)
        _refused(pkg, lambda: s.sens_hvp(D, dD, 1.0, 1.0), -1, "CR == CL")
        unchanged()
        # hv and curv may each be NULL
        assert L.deff_sensitivity_hvp_D(s._ctx, vp(D), vp(dD), CL, CR, None, None, None) == 0
        unchanged()
        # every call that replaces the system or the image invalidates the tangent: the pass refuses, the old map stays
        A, b = s.get_system()
        for again in (lambda: s.assemble_2phase(1e-3, 1.0, CL, CR), lambda: s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR),
                      lambda: s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR), lambda: s.assemble_from_D(D, CL, CR),
                      lambda: s.set_system(A, b, D, CL, CR), lambda: s.synth_image(1, 0),
                      lambda: s.set_image(oracle.synth_mask(nx, ny, 12345, 0))):
            s.set_image(oracle.synth_mask(nx, ny, 12345, 0))
            s.assemble_from_D(D, CL, CR)
            s.set_field(x)
            s.set_tangent(y)
            assert np.array_equal(s.sens_hvp(D, dD, CL, CR)[0], hv0)
            again()
            s.set_field(x)
            _refused(pkg, lambda: s.sens_hvp(D, dD, CL, CR), -5, "tangent")
            _refused(pkg, s.get_tangent, -5)
            unchanged()
    with pkg.SlabRank(nx + 1, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(oracle.synth_mask(nx + 1, ny, 12345, 0))
        sr.assemble_2phase(1e-3, 1.0, CL, CR)
        sr.init_linear(CL, CR)
        x0 = sr.get_field()
        out = np.zeros((ny, nx + 1))
        one = np.ones((ny, nx + 1))
        assert L.deff_sensitivity_hvp_D(sr._ctx, vp(one), vp(one), CL, CR, vp(out), None, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert L.deff_set_tangent(sr._ctx, vp(one)) == -1 and b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0) and np.all(out == 0.0)


# ---- torch ---------------------------------------------------------------------------------------------------------------

def test_torch_second_order(pkg):
    """effective_diffusivity twice differentiated, at 12 x 9 on cpu and cuda and on a stack of 2 on a passed solver:
    grad(create_graph=True) then (g * w).sum().backward() equals Solver.deff_hvp after the forward pass's calls made by hand
    (array_equal), torch.autograd.functional.hvp agrees with it, and it matches central differences of D.grad along w (bar:
    10 x the gap between the steps 1e-5 and 1e-6, the gap below 1e-4).  First-order backward is bitwise the library calls made
    by hand."""
    import torch
    from effectivediffusivityfvm_amd import effective_diffusivity
    nx, ny = 12, 9
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(13)
    Dn = np.exp(2.0 * rng.standard_normal((2, ny, nx)))
    wn = Dn * rng.standard_normal((2, ny, nx))

    def by_hand(s, D, w):
        nimg = D.shape[0] if D.ndim == 3 else 1
        s.assemble_from_D(D.reshape(nimg * ny, nx), CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        rs = s.solve_cg(rtol=1e-12)
        assert all(r.converged for r in (rs if isinstance(rs, list) else [rs]))
        g, _ = s.sensitivity(D.reshape(nimg * ny, nx), CL, CR)
        hv, _ = s.deff_hvp(D.reshape(nimg * ny, nx), w.reshape(nimg * ny, nx), CL, CR, rtol=1e-12)
        return np.asarray(g).reshape(D.shape), np.asarray(hv).reshape(D.shape)

    with pkg.Solver(nx, ny) as s:
        g_hand, hv_hand = by_hand(s, Dn[0], wn[0])
    assert np.any(hv_hand != 0.0)

    def grad_at(Dq, dev):
        Dt = torch.tensor(Dq, dtype=torch.float64, device=dev, requires_grad=True)
        effective_diffusivity(Dt, CL, CR).backward()
        return Dt.grad.cpu().numpy()

    for dev in ("cpu", "cuda"):
        D = torch.tensor(Dn[0], dtype=torch.float64, device=dev, requires_grad=True)
        w = torch.tensor(wn[0], dtype=torch.float64, device=dev)
        (g,) = torch.autograd.grad(effective_diffusivity(D, CL, CR), D, create_graph=True)
        assert g.requires_grad and np.array_equal(g.detach().cpu().numpy(), g_hand)
        (g * w).sum().backward()
        assert D.grad.shape == D.shape and D.grad.device == D.device and D.grad.dtype == torch.float64
        hv = D.grad.cpu().numpy()
        assert np.array_equal(hv, hv_hand)
        _, hv_f = torch.autograd.functional.hvp(lambda q: effective_diffusivity(q, CL, CR), D.detach(), w)
        assert np.array_equal(hv_f.cpu().numpy(), hv_hand)
        # first order: what it was, bitwise, and no graph without create_graph
        assert np.array_equal(grad_at(Dn[0], dev), g_hand)
        D1 = torch.tensor(Dn[0], dtype=torch.float64, device=dev, requires_grad=True)
        (g1,) = torch.autograd.grad(effective_diffusivity(D1, CL, CR), D1)
        assert not g1.requires_grad and np.array_equal(g1.cpu().numpy(), g_hand)
        fd5 = (grad_at(Dn[0] + 1e-5 * wn[0], dev) - grad_at(Dn[0] - 1e-5 * wn[0], dev)) / 2e-5
        fd6 = (grad_at(Dn[0] + 1e-6 * wn[0], dev) - grad_at(Dn[0] - 1e-6 * wn[0], dev)) / 2e-6
        scale = np.max(np.abs(hv))
        gap, err = np.max(np.abs(fd5 - fd6)) / scale, np.max(np.abs(hv - fd5)) / scale
        print(f"effective_diffusivity second order on {dev}: gap {gap:.3e} err {err:.3e}")
        assert gap < 1e-4, gap
        assert err <= 10.0 * gap, (err, gap)
    # a stack of 2 on a solver that is passed in and stays open
    with pkg.Solver(nx, ny, nimg=2) as s:
        g_hand2, hv_hand2 = by_hand(s, Dn, wn)
        D = torch.tensor(Dn, dtype=torch.float64, device="cuda", requires_grad=True)
        w = torch.tensor(wn, dtype=torch.float64, device="cuda")
        (g,) = torch.autograd.grad(effective_diffusivity(D, CL, CR, solver=s).sum(), D, create_graph=True)
        s.init_linear(CL, CR)                            # whatever happens to the passed solver in between
        (g * w).sum().backward()
        s.init_linear(CL, CR)                            # the passed solver is still open
        _, hv_f = torch.autograd.functional.hvp(lambda q: effective_diffusivity(q, CL, CR, solver=s).sum(), D.detach(), w)
    assert np.array_equal(g.detach().cpu().numpy(), g_hand2)
    assert np.array_equal(D.grad.cpu().numpy(), hv_hand2) and np.array_equal(hv_f.cpu().numpy(), hv_hand2)
