"""The Deff gradient of a volume on the GPU (deff_volume_sensitivity_D, k_sens3): the map bit for bit against the numpy model
(volume_sens_model.py) at every launch geometry, a volume of one slice against the 2-D pass, a converged field end to end
against a dense solve, that the pass changes no other state, the refusals, and the torch op effective_diffusivity_volume."""
import ctypes as C
import functools

import numpy as np
import pytest

import volume_model as vm
from test_cg_host import rel_l2
from test_gpu_sensitivity import device_rows
from volume_sens_model import sensitivity3

pytestmark = pytest.mark.gpu

WALLS = [(0.0, 1.0), (2.0, -1.0)]
EINVAL, ESTATE = -1, -5
EULER_REL = 1e-13              # the fixed-order double sum against the model's long-double sum

SHAPES = [(2, 2, 1), (2, 2, 2),                     # smallest volumes
          (3, 2, 9),                                # every row is a slice's first or last
          (9, 7, 3),                                # odd width, pad column, slice borders inside tiles
          (16, 3, 5),                               # several borders per tile, z neighbours inside the same tile
          (6, 8, 4),                                # slices aligned with tiles
          (129, 4, 3), (130, 5, 4),                 # a last strip of 1 and 2 columns
          (258, 9, 2),                              # a third strip
          (130, 71, 3),                             # a larger two-strip case
          (5, 40, 3),                               # z rows five tiles away
          (2, 2, 33000)]                            # 66 000 rows: the planner itself picks sens_kt 2


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


@functools.lru_cache(maxsize=None)
def case(nx, ny, nz):
    """(x, D) of a shape: a seeded field that is no solution of anything, seeded_D with 10 % zeros.  Computed once, never
    written."""
    D = vm.seeded_D(nx, ny, nz)
    x = np.random.default_rng(31 * nx + 7 * ny + nz).uniform(-0.5, 2.5, (nz, ny, nx))
    for a in (x, D):
        a.setflags(write=False)
    return x, D


@functools.lru_cache(maxsize=None)
def model(nx, ny, nz, CL, CR):
    g, e = sensitivity3(*case(nx, ny, nz), CL, CR)
    g.setflags(write=False)
    return g, e


def check_against_model(v, nx, ny, nz, CL, CR):
    x, D = case(nx, ny, nz)
    g_ref, e_ref = model(nx, ny, nz, CL, CR)
    g, e = v.sensitivity(D, CL, CR)
    rel = abs(np.longdouble(e) - e_ref) / abs(e_ref)
    print(f"({nx},{ny},{nz}) walls ({CL}, {CR}) kt {v.plan_value('sens_kt')} items {v.plan_value('sens_items')}: "
          f"map equal {np.array_equal(g, g_ref)}  euler rel {float(rel):.3e}")
    assert g.shape == (nz, ny, nx) and np.array_equal(g, g_ref)
    assert rel <= EULER_REL, (e, e_ref)
    return g, e


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Bit for bit against the model

@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_map_has_the_models_bits(pkg, nx, ny, nz, CL, CR):
    x, D = case(nx, ny, nz)
    assert (D == 0).any() or D.size < 16
    with pkg.Volume(nx, ny, nz) as v:
        v.set_field(x)
        g, e = check_against_model(v, nx, ny, nz, CL, CR)
        if nz == 33000:
            assert v.plan_value("sens_kt") == 2
        g2, e2 = v.sensitivity(D, CL, CR)                           # a second call: the same bits
        assert vm.same_bits(g2, g) and e2 == e
        assert vm.same_bits(v.get_field(), x)


@pytest.mark.parametrize("nx,ny,nz,items", [(130, 5, 4, (6, 4, 2)),           # 20 rows, 3 tiles, 2 strips
                                            (5, 40, 3, (15, 8, 1))])         # 120 rows, 15 tiles
def test_every_run_length_against_the_model(pkg, nx, ny, nz, items):
    x, D = case(nx, ny, nz)
    CL, CR = WALLS[1]
    tiles = -(-ny * nz // 8)
    with pkg.Volume(nx, ny, nz) as v:
        v.set_field(x)
        for kt, want in zip((1, 2, 64), items):
            v.set_tuning("sens_kt", kt)
            check_against_model(v, nx, ny, nz, CL, CR)
            assert v.plan_value("sens_kt") == min(kt, tiles) and v.plan_value("sens_items") == want, (kt, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. One slice is the 2-D pass

@pytest.mark.parametrize("nx,ny", [(9, 7), (130, 33), (258, 9)])
def test_one_slice_is_the_2d_pass(pkg, nx, ny):
    x, D = case(nx, ny, 1)
    for CL, CR in WALLS:
        with pkg.Solver(nx, ny) as s, pkg.Volume(nx, ny, 1) as v:
            s.set_field(x[0])
            v.set_field(x)
            g2, e2 = s.sensitivity(D[0], CL, CR)
            g3, e3 = v.sensitivity(D, CL, CR)
            assert vm.same_bits(g3[0], g2) and e3 == e2, (e3, e2)
            for key in ("sens_kt", "sens_items"):
                assert v.plan_value(key) == s.plan_value(key), key


# ---------------------------------------------------------------------------------------------------------------------------
# 3. A converged field, end to end (the rule of test_gpu_volume.py::test_fixed_point_is_the_dense_solve: max(1e-10, 10 d_ref),
#    d_ref = the same distance for numpy's float64 CG from the same guess to the same rtol)

@pytest.mark.parametrize("nx,ny,nz", [(9, 7, 3), (12, 10, 6), (33, 5, 4)])
def test_converged_field_end_to_end(pkg, nx, ny, nz):
    rtol, CL, CR = 1e-13, 0.25, 1.5
    D = np.exp(np.random.default_rng(1000003 * nx + 1009 * ny + nz).standard_normal((nz, ny, nx)))
    A, b = vm.rows3(D, CL, CR)
    xd = np.linalg.solve(vm.dense3(A, D.shape), b).reshape(D.shape)
    g_ref, _ = sensitivity3(xd, D, CL, CR)
    deff_exact = vm.deff_of(xd, D, CL, CR)
    with pkg.Volume(nx, ny, nz) as v:
        v.assemble_from_D(D, CL, CR)
        v.init_linear(CL, CR)
        x0 = v.get_field()
        r = v.solve_cg(rtol=rtol)
        assert r.converged and r.iters > 0, r
        g, e = v.sensitivity(D, CL, CR)
    fields, k = vm.pcg(A, b, x0, D.shape, 1_000_000, np.float64, rtol=rtol)
    g_np, e_np = sensitivity3(fields[k], D, CL, CR)
    d_ref = rel_l2(g_np, g_ref)
    e_ref = abs(float(e_np) - vm.deff_of(fields[k], D, CL, CR)) / abs(deff_exact)
    d_gpu = rel_l2(g, g_ref)
    e_gpu = abs(e - r.deff_raw) / abs(deff_exact)
    print(f"volume sensitivity end to end ({nx},{ny},{nz}): numpy CG {k} iterations d_ref {d_ref:.3e} euler-deff {e_ref:.3e}; "
          f"GPU {r.iters} iterations d {d_gpu:.3e} euler-deff {e_gpu:.3e}")
    assert d_gpu <= max(1e-10, 10 * d_ref), (d_gpu, d_ref)
    assert e_gpu <= max(1e-10, 10 * e_ref), (e_gpu, e_ref)
    assert abs(e - deff_exact) <= max(1e-10, 10 * e_ref) * abs(deff_exact)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. The pass changes no other state

def test_the_pass_changes_no_other_state(pkg):
    nx, ny, nz = 16, 3, 5
    CL, CR = 0.25, 1.5
    D = vm.seeded_D(nx, ny, nz)

    def run(with_pass):
        with pkg.Volume(nx, ny, nz) as v:
            v.assemble_from_D(D, CL, CR)
            v.init_linear(CL, CR)
            sys0 = v.get_system()
            r1 = v.solve_cg(rtol=1e-12, max_iter=5)
            if with_pass:
                x5 = v.get_field()
                v.sensitivity(D, CL, CR)
                assert vm.same_bits(v.get_field(), x5)
                assert all(vm.same_bits(a, c) for a, c in zip(v.get_system(), sys0))
            r2 = v.solve_cg(rtol=1e-12)
            assert all(vm.same_bits(a, c) for a, c in zip(v.get_system(), sys0))
            return (r1.iters, r1.deff_raw, r2.iters, r2.deff_raw, r2.rel_residual, r2.converged), v.get_field()

    plain, with_pass = run(False), run(True)
    assert plain[0][0] == 5 and plain[0][5] and plain[0][2] > 0
    assert with_pass[0] == plain[0] and vm.same_bits(with_pass[1], plain[1])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Refusals

def test_refusals_leave_field_and_map_alone(pkg):
    nx, ny, nz = 9, 7, 3                                  # odd width: the device map has a pad column
    CL, CR = 0.0, 1.0
    x, D = case(nx, ny, nz)
    L = pkg._capi.load()
    err = lambda: L.deff_last_error().decode()
    Dp = np.ascontiguousarray(D).ctypes.data_as(C.c_void_p)
    e = C.c_double()
    assert L.deff_volume_sensitivity_D(None, Dp, CL, CR, None, C.byref(e), None) == EINVAL
    with pkg.Volume(nx, ny, nz) as v:
        hv = v._vol
        with pytest.raises(pkg.DeffError) as ei:
            v.device_sensitivity_ptr()
        assert ei.value.code == ESTATE and "no sensitivity map yet" in err()
        # the order of the refusals: a NULL D before the missing field, the missing field before the walls
        assert L.deff_volume_sensitivity_D(hv, None, CL, CR, None, C.byref(e), None) == EINVAL and "D is NULL" in err()
        assert L.deff_volume_sensitivity_D(hv, Dp, 1.0, 1.0, None, C.byref(e), None) == ESTATE and "no field" in err()
        with pytest.raises(pkg.DeffError) as ei:
            v.device_sensitivity_ptr()
        assert ei.value.code == ESTATE
        v.set_field(x)                                                    # a field, no system: the map needs none
        g0, e0 = v.sensitivity(D, CL, CR)
        assert np.array_equal(g0, model(nx, ny, nz, CL, CR)[0])
        p0, pitch = v.device_sensitivity_ptr()
        assert pitch == 8 * (nx + 1)
        dev0 = device_rows(p0, ny * nz, pitch)
        assert np.array_equal(dev0[:, :nx].reshape(nz, ny, nx), g0) and np.all(dev0[:, nx] == 0.0)

        def unchanged():
            p, pt = v.device_sensitivity_ptr()
            assert (p, pt) == (p0, pitch) and vm.same_bits(device_rows(p, ny * nz, pt), dev0)
            assert vm.same_bits(v.get_field(), x)

        assert L.deff_volume_sensitivity_D(hv, None, CL, CR, None, C.byref(e), None) == EINVAL and "D is NULL" in err()
        unchanged()
        with pytest.raises(pkg.DeffError) as ei:
            v.sensitivity(D, 1.0, 1.0)
        assert ei.value.code == EINVAL and "deff_volume_sensitivity_D: CR == CL" in err()
        unchanged()
        for key in ("cg_kr", "res_kt", "sens_items", ""):
            with pytest.raises(pkg.DeffError) as ei:
                v.set_tuning(key, 1)
            assert ei.value.code == EINVAL and f"'{key}'" in err(), key
            unchanged()
        with pytest.raises(pkg.DeffError) as ei:
            v.set_tuning("sens_kt", -1)
        assert ei.value.code == EINVAL
        with pytest.raises(pkg.DeffError) as ei:
            v.plan_value("vjp_kt")
        assert ei.value.code == EINVAL
        unchanged()
        # g, euler and ms may each be NULL
        assert L.deff_volume_sensitivity_D(hv, Dp, CL, CR, None, None, None) == 0
        unchanged()
        g, e1, ms = v.sensitivity(D, CL, CR, timing=True)
        assert vm.same_bits(g, g0) and e1 == e0 and ms > 0.0


def test_a_volumes_pass_leaves_a_2d_solver_alone(pkg):
    nx, ny = 130, 33
    CL, CR = WALLS[1]
    x2, D2 = case(nx, ny, 1)

    def run_2d(s):
        g, e = s.sensitivity(D2[0], CL, CR)
        return g, e, s.plan_value("sens_kt"), s.plan_value("sens_items")

    def same(a, b):
        return vm.same_bits(a[0], b[0]) and a[1:] == b[1:]

    with pkg.Solver(nx, ny) as s:
        s.set_field(x2[0])
        before = run_2d(s)
        with pkg.Volume(16, 3, 5) as v:
            v.set_field(case(16, 3, 5)[0])
            v.set_tuning("sens_kt", 1)
            check_against_model(v, 16, 3, 5, CL, CR)
            assert same(run_2d(s), before)
            assert vm.same_bits(s.get_field(), x2[0])
        assert same(run_2d(s), before)
    with pkg.Solver(nx, ny) as s:
        s.set_field(x2[0])
        assert same(run_2d(s), before)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. The torch op

def test_torch_op(pkg):
    import torch
    import torch.autograd.forward_ad as fwAD
    nz, ny, nx = 3, 4, 5
    CL, CR = 0.25, 1.5
    rng = np.random.default_rng(345)
    Dn = np.exp(rng.standard_normal((nz, ny, nx)))
    tn = rng.standard_normal((nz, ny, nx))
    with pkg.Volume(nx, ny, nz) as v:
        v.assemble_from_D(Dn, CL, CR)
        v.init_linear(CL, CR)
        r = v.solve_cg(rtol=1e-10)
        g_ref, _ = v.sensitivity(Dn, CL, CR)
    for dev in ("cpu", "cuda"):
        D = torch.tensor(Dn, dtype=torch.float64, device=dev, requires_grad=True)
        out = pkg.effective_diffusivity_volume(D, CL, CR)
        assert out.shape == () and out.device == D.device and out.item() == r.deff_raw
        (-2.0 * out).backward()
        assert D.grad.device == D.device and np.array_equal(D.grad.cpu().numpy(), -2.0 * g_ref)
        t = torch.tensor(tn, dtype=torch.float64, device=dev)
        with fwAD.dual_level():
            e, de = fwAD.unpack_dual(pkg.effective_diffusivity_volume(fwAD.make_dual(D.detach(), t), CL, CR))
        assert e.item() == r.deff_raw and de.device == D.device
        assert de.item() == (torch.tensor(g_ref, device=dev) * t).sum().item()
        # once differentiable: torch refuses the second backward pass, no constant comes out silently
        D2 = torch.tensor(Dn, dtype=torch.float64, device=dev, requires_grad=True)
        (gD,) = torch.autograd.grad(pkg.effective_diffusivity_volume(D2, CL, CR), D2, create_graph=True)
        assert np.array_equal(gD.detach().cpu().numpy(), g_ref)
        with pytest.raises(RuntimeError):
            gD.sum().backward()
        assert D2.grad is None
    # a passed volume is used and kept; one of the wrong shape is refused
    D = torch.tensor(Dn, dtype=torch.float64, requires_grad=True)
    with pkg.Volume(nx, ny, nz) as v:
        out = pkg.effective_diffusivity_volume(D, CL, CR, volume=v)
        assert out.item() == r.deff_raw and vm.same_bits(device_map(v, nx, ny, nz), g_ref)
    with pkg.Volume(nx, nz, ny) as v, pytest.raises(ValueError):
        pkg.effective_diffusivity_volume(D, CL, CR, volume=v)
    with pytest.raises(TypeError):
        pkg.effective_diffusivity_volume(D[0], CL, CR)
    # CG that does not converge: the 2-D op's sentence under the new name
    with pytest.raises(RuntimeError, match="effective_diffusivity_volume: CG did not converge"):
        pkg.effective_diffusivity_volume(D, CL, CR, max_iter=1)


def device_map(v, nx, ny, nz):
    p, pitch = v.device_sensitivity_ptr()
    return device_rows(p, ny * nz, pitch)[:, :nx].reshape(nz, ny, nx)
