"""The Deff gradient on the GPU (deff_sensitivity / deff_sensitivity_D, csrc/kernels_sens.hpp): the map bit for bit against the
numpy model of the normative expressions at every strip / seam / pad shape, the Euler sum, the image form, a converged field end
to end, refusals, the absence of side effects and the torch op."""
import ctypes as C

import numpy as np
import pytest

from sensitivity_model import sensitivity as model
from test_cg_host import block_thomas, pcg_numpy, rel_l2

pytestmark = pytest.mark.gpu

WALLS = [(0.0, 1.0), (2.0, -1.0)]


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def make_case(nx, ny, nimg, CL, CR, seed):
    """A smooth-plus-random field (no solve needed: the map is a function of any field) and D = exp(2 N(0, 1)) with zeros,
    some of them on the walls and next to each other."""
    rng = np.random.default_rng(seed)
    j = (np.arange(nx) + 0.5) / nx
    i = (np.arange(ny) + 0.5) / ny
    x = CL + (CR - CL) * j[None, None, :] + 0.1 * np.sin(3.0 * i)[None, :, None] * np.cos(2.0 * j)[None, None, :]
    x = x + 0.05 * rng.standard_normal((nimg, ny, nx))
    D = np.exp(2.0 * rng.standard_normal((nimg, ny, nx)))
    D[rng.random((nimg, ny, nx)) < 0.06] = 0.0
    D[:, 0, 0] = 0.0
    D[:, ny - 1, nx - 1] = 0.0
    if nx > 2:
        D[:, ny // 2, nx // 2 - 1:nx // 2 + 1] = 0.0
    return x, D


def model_stack(x, D, CL, CR):
    out = [model(x[k], D[k], CL, CR) for k in range(x.shape[0])]
    return np.stack([g for g, _ in out]), [e for _, e in out]


def check_map(pkg, nx, ny, nimg, CL, CR, kt=0, seed=0):
    """The map equals the model's (array_equal), the Euler sums are within 1e-13 of the model's long-double sums and the same
    bits on a second call.  Returns (sens_kt, sens_items) as used."""
    x, D = make_case(nx, ny, nimg, CL, CR, seed)
    want, euler_want = model_stack(x, D, CL, CR)
    with pkg.Solver(nx, ny, nimg=nimg) as s:
        s.set_field(x.reshape(nimg * ny, nx))
        if kt:
            s.set_tuning("sens_kt", kt)
        g, e = s.sensitivity(D.reshape(nimg * ny, nx), CL, CR)
        g2, e2 = s.sensitivity(D.reshape(nimg * ny, nx), CL, CR)
        plan = s.plan_value("sens_kt"), s.plan_value("sens_items")
    g, g2 = g.reshape(nimg, ny, nx), g2.reshape(nimg, ny, nx)
    e, e2 = np.atleast_1d(e), np.atleast_1d(e2)
    for k in range(nimg):
        bad = np.argwhere(g[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), g[k][tuple(bad[0])], want[k][tuple(bad[0])])
        rel = abs(float(np.longdouble(e[k]) - euler_want[k])) / abs(float(euler_want[k]))
        print(f"sensitivity {nimg} x {nx}x{ny} kt {plan[0]} image {k}: euler rel {rel:.3e}")
        assert rel <= 1e-13, (k, e[k], euler_want[k])
    assert np.array_equal(g, g2) and np.array_equal(e, e2)
    assert np.all(g[D == 0.0] == 0.0)
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
    """"sens_kt": 9 tile rows, 2 strips -- kt = 1 has a seam every 8 rows (9 items per strip), kt = 2 every 16 (5 items, the last
    one 7 rows short), kt = 64 is clipped to the image (one item per strip, no seam)."""
    used, items = check_map(pkg, nx, ny, nimg, 0.0, 1.0, kt=kt, seed=7 + kt)
    assert (used, items) == {1: (1, 18), 2: (2, 10), 64: (9, 2)}[kt]


def test_map_matches_model_large(pkg):
    """2050 x 1537: 17 strips (the last one 2 columns wide), 193 tile rows, an odd height."""
    kt, items = check_map(pkg, 2050, 1537, 1, 0.0, 1.0, seed=99)
    assert items == 17 * ((193 + kt - 1) // kt)


@pytest.mark.parametrize("phases", [2, 3])
def test_image_form_equals_plane_form(pkg, oracle, phases):
    """deff_sensitivity fills the D plane on the device from the stored phase diffusivities: the bits of deff_sensitivity_D on
    the oracle's fill_D_* plane.  2-phase: a 97 x 41 image amplified 2 x 3; 3-phase without a Grid: the image as it is (odd
    width: a pad column), a gas phase that cannot diffuse."""
    rng = np.random.default_rng(phases)
    pix = rng.integers(0, 256, (41, 97), dtype=np.uint8)
    CL, CR = 2.0, -1.0
    if phases == 2:
        ax, ay = 2, 3
        D = oracle.fill_D_2phase(pix, 1.0, 1e-3, ax, ay)
    else:
        ax, ay = 1, 1
        D = oracle.fill_D_3phase(pix, 1.0, 1e-3, 0.0)
    ny, nx = D.shape
    x, _ = make_case(nx, ny, 1, CL, CR, 11)
    with pkg.Solver(nx, ny) as s:
        s.set_image(pix, ax, ay)
        if phases == 2:
            s.assemble_2phase(1e-3, 1.0, CL, CR)
        else:
            s.assemble_3phase(1e-3, 1.0, 0.0, CL, CR)
        s.set_field(x[0])
        g, e = s.sensitivity()
        gD, eD = s.sensitivity(D, CL, CR)
    want, _ = model(x[0], D, CL, CR)
    assert np.array_equal(g, gD) and e == eD
    assert np.array_equal(g, want)
    assert np.any(g > 0.0)


@pytest.mark.parametrize("nx,ny", [(40, 32), (130, 71)])
def test_converged_field_end_to_end(pkg, oracle, nx, ny):
    """assemble_from_D + solve_cg(rtol 1e-13) + sensitivity_D against the model on the direct solve's field.  Bars as in
    test_gpu_cg.py: max(1e-10, 10 d_ref), d_ref the same distance for numpy's float64 CG stopped at the same rtol; the Euler
    sum against deff_raw under the same rule."""
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    A, b = oracle.discretize(D, CL, CR)
    xd = block_thomas(A, b, nx, ny)
    g_ref, _ = model(xd, D, CL, CR)
    deff_exact = oracle.flux_deff(xd, D, CL, CR)[0]
    t = pcg_numpy(A, b, oracle.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-13)
    g_np, euler_np = model(t.x, D, CL, CR)
    d_ref = rel_l2(g_np, g_ref)
    e_ref = abs(float(euler_np) - oracle.flux_deff(t.x, D, CL, CR)[0]) / abs(deff_exact)
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(D, CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        r = s.solve_cg(rtol=1e-13)
        g, e = s.sensitivity(D, CL, CR)
    d_gpu = rel_l2(g, g_ref)
    e_gpu = abs(e - r.deff_raw) / abs(deff_exact)
    print(f"sensitivity end to end {nx}x{ny}: numpy CG {t.iters} iterations d_ref {d_ref:.3e} euler-deff {e_ref:.3e}; "
          f"GPU {r.iters} iterations d {d_gpu:.3e} euler-deff {e_gpu:.3e}")
    assert d_gpu <= max(1e-10, 10 * d_ref), (d_gpu, d_ref)
    assert e_gpu <= max(1e-10, 10 * e_ref), (e_gpu, e_ref)
    assert abs(e - deff_exact) <= max(1e-10, 10 * e_ref) * abs(deff_exact)


def device_rows(ptr, rows, pitch_bytes):
    """rows x (pitch_bytes / 8) doubles from a device pointer, copied by the HIP runtime the library itself runs on."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    assert path, "no HIP runtime mapped into this process"
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    assert pitch_bytes % 8 == 0
    out = np.full((rows, pitch_bytes // 8), np.nan)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def _refused(pkg, fn, code, word=None):
    with pytest.raises(pkg.DeffError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    if word:
        assert word in str(ei.value), ei.value


def test_refusals_leave_field_and_map_alone(pkg, oracle):
    nx, ny = 33, 20                                       # odd width: the device map has a pad column
    CL, CR = 0.0, 1.0
    x, D = make_case(nx, ny, 1, CL, CR, 3)
    x, D = x[0], D[0]
    pix = oracle.synth_mask(nx, ny, 12345, 0)
    L = pkg._capi.load()
    with pkg.Solver(nx, ny) as s:
        _refused(pkg, s.device_sensitivity_ptr, -5)      # DEFF_ESTATE: no map yet
        _refused(pkg, lambda: s.sensitivity(D, CL, CR), -5, "no field")
        s.set_field(x)
        g0, e0 = s.sensitivity(D, CL, CR)
        p0, pitch = s.device_sensitivity_ptr()
        assert pitch == 8 * (nx + 1)
        dev0 = device_rows(p0, ny, pitch)
        assert np.array_equal(dev0[:, :nx], g0) and np.all(dev0[:, nx] == 0.0)

        def unchanged():
            p, pt = s.device_sensitivity_ptr()
            assert (p, pt) == (p0, pitch) and np.array_equal(device_rows(p, ny, pt), dev0)
            assert np.array_equal(s.get_field(), x)

        _refused(pkg, lambda: s.sensitivity(D, 1.0, 1.0), -1, "CR == CL")
        unchanged()
        e = (C.c_double * 1)()
        assert L.deff_sensitivity_D(s._ctx, None, CL, CR, None, e, None) == -1 and b"D is NULL" in L.deff_last_error()
        unchanged()
        _refused(pkg, s.sensitivity, -5)                 # no assembled image system
        unchanged()
        s.assemble_from_D(D, CL, CR)
        s.set_field(x)
        _refused(pkg, s.sensitivity, -5)                 # a D plane is no image system
        unchanged()
        A, b = oracle.discretize(np.where(D == 0, 1.0, D), CL, CR)
        s.set_system(A, b, None, CL, CR)
        s.set_field(x)
        _refused(pkg, s.sensitivity, -5)
        unchanged()
        s.set_image(pix)
        s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR, grid=np.zeros((ny, nx), dtype=np.uint32))
        s.set_field(x)
        _refused(pkg, s.sensitivity, -1, "Grid")
        unchanged()
        s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR)
        s.set_field(x)
        _refused(pkg, s.sensitivity, -1, "Grid")
        unchanged()
        s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR)        # ... and without a Grid the same context goes through
        s.set_field(x)
        g, _ = s.sensitivity()
        assert np.array_equal(g, model(x, oracle.fill_D_3phase(pix, 1.0, 1e-3, 10.0), CL, CR)[0])
        # g and euler may each be NULL
        assert L.deff_sensitivity_D(s._ctx, np.ascontiguousarray(D).ctypes.data_as(C.c_void_p), CL, CR, None, None, None) == 0
        assert np.array_equal(device_rows(s.device_sensitivity_ptr()[0], ny, pitch), dev0)     # the map of (x, D) again
    with pkg.SlabRank(nx + 1, ny, 0, 1, pkg.rccl_unique_id()) as sr:
        sr.set_image(oracle.synth_mask(nx + 1, ny, 12345, 0))
        sr.assemble_2phase(1e-3, 1.0, CL, CR)
        sr.init_linear(CL, CR)
        x0 = sr.get_field()
        Dn = np.ones((ny, nx + 1))
        out = np.zeros((ny, nx + 1))
        e = (C.c_double * 1)()
        assert L.deff_sensitivity_D(sr._ctx, Dn.ctypes.data_as(C.c_void_p), CL, CR, out.ctypes.data_as(C.c_void_p), e, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert L.deff_sensitivity(sr._ctx, out.ctypes.data_as(C.c_void_p), e, None) == -1
        assert b"row-slab" in L.deff_last_error()
        assert np.array_equal(sr.get_field(), x0) and np.all(out == 0.0)


@pytest.mark.parametrize("form", ["resident", "streaming"])
def test_no_side_effects_on_a_jacobi_run(pkg, form):
    """sweeps(27) + solve(...) with a sensitivity call in between (it settles the pending resident interval) gives the bits it
    gives without the call, and the solve's loop_ms stays a time: the call uses an event pair of its own."""
    nx, ny = 256, 192
    runs = []
    for call in (False, True):
        with pkg.Solver(nx, ny, kernel="matfree_tb") as s:
            if form == "streaming":
                s.set_tuning("tb_impl", 1)
            s.synth_image(12345, 0)
            s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
            s.init_linear(0.0, 1.0)
            s.sweeps(27)
            if call:
                g, e, ms = s.sensitivity(timing=True)
                assert np.all(np.isfinite(g)) and np.isfinite(e) and ms > 0.0
            r = s.solve(1e-9, 101, check_every=50)
            p = s.plan()
            print(f"{form}: plan {p}")
            assert p["tb_impl"] == (2 if form == "resident" else 1), p
            assert np.isfinite(r.loop_ms) and r.loop_ms > 0.0, r
            runs.append((s.get_field(), r.iters, r.checks, r.deff_raw, r.conv, s.plan_value("tb_fallbacks")))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1:] == runs[1][1:], (runs[0][1:], runs[1][1:])


def test_torch_op(pkg, oracle):
    """effective_diffusivity at 12 x 9: forward = solve_cg's deff_raw, backward = the model's map on the direct solve's field
    within the end-to-end bar, a stack of 2, outputs on the input's device."""
    import torch
    from effectivediffusivityfvm_amd.autograd import effective_diffusivity
    nx, ny = 12, 9
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(12)
    Dn = np.exp(2.0 * rng.standard_normal((2, ny, nx)))
    refs = []
    for k in range(2):
        A, b = oracle.discretize(Dn[k], CL, CR)
        xd = block_thomas(A, b, nx, ny)
        g_ref, _ = model(xd, Dn[k], CL, CR)
        t = pcg_numpy(A, b, oracle.linear_guess(nx, ny, CL, CR), nx, ny, 50_000, np.float64, rtol=1e-12)
        refs.append((g_ref, rel_l2(model(t.x, Dn[k], CL, CR)[0], g_ref)))
    with pkg.Solver(nx, ny) as s:
        s.assemble_from_D(Dn[0], CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        deff0 = s.solve_cg(rtol=1e-12).deff_raw
    for dev in ("cpu", "cuda"):
        D = torch.tensor(Dn[0], dtype=torch.float64, device=dev, requires_grad=True)
        out = effective_diffusivity(D, CL, CR)
        assert out.shape == () and out.device == D.device and out.dtype == torch.float64
        assert out.item() == deff0
        (3.0 * out).backward()
        assert D.grad.device == D.device and D.grad.shape == D.shape
        d = rel_l2(D.grad.cpu().numpy() / 3.0, refs[0][0])
        print(f"torch op on {dev}: backward {d:.3e} from the model on the direct solve (numpy CG {refs[0][1]:.3e})")
        assert d <= max(1e-10, 10 * refs[0][1]), (d, refs[0][1])
    D = torch.tensor(Dn, dtype=torch.float64, device="cuda", requires_grad=True)
    with pkg.Solver(nx, ny, nimg=2) as s:
        s.assemble_from_D(Dn.reshape(2 * ny, nx), CL, CR)
        s.init_linear(CL, CR)
        s.set_tuning("cg_planes", 1)
        deff2 = [r.deff_raw for r in s.solve_cg(rtol=1e-12)]
        out = effective_diffusivity(D, CL, CR, solver=s)
        assert out.shape == (2,) and out.device == D.device
        assert out.tolist() == deff2 and abs(deff2[0] - deff0) <= 1e-10 * abs(deff0)
        (out * torch.tensor([1.0, -2.0], dtype=torch.float64, device="cuda")).sum().backward()
        s.init_linear(CL, CR)                            # the passed solver is still open
    grad = D.grad.cpu().numpy()
    for k, w in enumerate((1.0, -2.0)):
        d = rel_l2(grad[k] / w, refs[k][0])
        assert d <= max(1e-10, 10 * refs[k][1]), (k, d, refs[k][1])
    with pytest.raises(RuntimeError, match="did not converge"):
        effective_diffusivity(torch.tensor(Dn[0], dtype=torch.float64), CL, CR, max_iter=2)
