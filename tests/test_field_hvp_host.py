"""The second-order field adjoint (deff_field_vjp_hvp_D and the adjoint's tangent), host side: the library's exports, the numpy
model of the normative expressions (tests/field_hvp_model.py) against central finite differences of the field adjoint's model
on direct solves, the identities that need no reference (S_w D = -g, symmetry, linearity in w), cells that cannot diffuse, and
the kernels' register / scratch / LDS budget on the ISA hipcc emits for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from field_hvp_model import field_hvp
from field_vjp_model import field_vjp
from tangent_model import tangent_rhs
from test_cg_host import block_thomas
from test_kernel_resources import remarks_of

NEW_SYMBOLS = ("deff_adjoint_tangent_rhs_D", "deff_solve_adjoint_tangent", "deff_get_adjoint_tangent",
               "deff_device_adjoint_tangent", "deff_set_adjoint_tangent", "deff_field_vjp_hvp_D", "deff_device_field_vjp_hvp")
SHAPES = [(5, 7), (6, 4)]                                # nx, ny: non-square cells
WALLS = [(0.0, 1.0), (2.0, -1.0)]


def test_library_exports_field_hvp():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("fhvp_kt", "fhvp_items"):
        assert f'"{key}"' in header, key
    for m in ("adjoint_tangent_rhs", "solve_adjoint_tangent", "get_adjoint_tangent", "set_adjoint_tangent", "field_vjp_hvp",
              "field_hvp"):
        assert callable(getattr(pkg.Solver, m)), m
    # argument checks come before any device work
    assert L.deff_adjoint_tangent_rhs_D(None, None, None, None, None, None) == -1
    assert L.deff_solve_adjoint_tangent(None, 1e-10, 10, 1, None) == -1
    assert L.deff_get_adjoint_tangent(None, None) == -1
    assert L.deff_device_adjoint_tangent(None, None, None) == -1
    assert L.deff_set_adjoint_tangent(None, None) == -1
    assert L.deff_field_vjp_hvp_D(None, None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_device_field_vjp_hvp(None, None, None) == -1


def _case(nx, ny):
    rng = np.random.default_rng(3000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    v = D * rng.standard_normal((ny, nx))                # a direction of D's own size per cell
    u = D * rng.standard_normal((ny, nx))
    w = rng.standard_normal((ny, nx))
    return D, v, u, w


def _zero_case():
    """12 x 9 with D == 0 cells on either wall, side by side, and two that cut the corner cell (8, 11) off."""
    nx, ny = 12, 9
    rng = np.random.default_rng(7)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    zero = np.zeros((ny, nx), dtype=bool)
    zero[1, 2] = zero[1, 3] = zero[4, 0] = zero[3, 11] = True
    zero[8, 10] = zero[7, 11] = True
    D[zero] = 0.0
    return D, zero, rng.standard_normal((ny, nx)), rng.standard_normal((ny, nx)), rng.standard_normal((ny, nx))


def _gradient(oracle, D, w, CL, CR, fixed=None):
    """The field adjoint's model g = grad of w^T x(D) on the direct solves of D, with w fixed."""
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    x = block_thomas(A, b, nx, ny, fixed=fixed)
    lam = block_thomas(A, w.ravel(), nx, ny, fixed=fixed)
    return field_vjp(x, lam, D, CL, CR)[0]


def _planes(oracle, D, v, w, CL, CR, fixed=None):
    """x = A^-1 b, lambda = A^-1 w, y = A^-1 r with r the tangent's expressions on x, m = A^-1 q with q the same on lambda and
    walls 0: the four planes of the pass on direct solves."""
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    x = block_thomas(A, b, nx, ny, fixed=fixed)
    lam = block_thomas(A, w.ravel(), nx, ny, fixed=fixed)
    r, _ = tangent_rhs(x, D, v, CL, CR)
    q, _ = tangent_rhs(lam, D, v, 0.0, 0.0)
    y = block_thomas(A, r.ravel(), nx, ny, fixed=fixed)
    m = block_thomas(A, q.ravel(), nx, ny, fixed=fixed)
    return x, lam, y, m


def _hvp(oracle, D, v, w, CL, CR, fixed=None):
    """The model's S_w v on direct solves."""
    return field_hvp(*_planes(oracle, D, v, w, CL, CR, fixed), D, v, CL, CR)


def _fd(oracle, D, v, w, CL, CR, h, fixed=None):
    return (_gradient(oracle, D + h * v, w, CL, CR, fixed) - _gradient(oracle, D - h * v, w, CL, CR, fixed)) / (2.0 * h)


def _against_fd(oracle, D, v, w, CL, CR, what, fixed=None):
    hv = _hvp(oracle, D, v, w, CL, CR, fixed)[0]
    fd5, fd6 = _fd(oracle, D, v, w, CL, CR, 1e-5, fixed), _fd(oracle, D, v, w, CL, CR, 1e-6, fixed)
    scale = np.max(np.abs(hv))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(hv - fd6)) / scale
    print(f"field hvp fd {what}: gap {gap:.3e} err {err:.3e}")
    # a wrong term, weight or sign shifts entries by O(1) of the largest one: the differences must be usable for the bar to tell
    assert scale > 0.0 and gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_against_finite_differences(oracle, nx, ny, CL, CR):
    """S_w v against central differences of field_vjp(x(D +- h v), lambda(D +- h v), D +- h v) with w fixed.  Bar: 10 x the gap
    between the differences at the steps 1e-5 and 1e-6 -- the finite differences' own uncertainty, the rule of
    test_sensitivity_host.py -- relative to the largest entry of S_w v, and the gap itself below 1e-4."""
    D, v, _, w = _case(nx, ny)
    _against_fd(oracle, D, v, w, CL, CR, f"{nx}x{ny} walls ({CL}, {CR})")


def test_model_against_finite_differences_with_zero_cells(oracle):
    """The same on 12 x 9 with cells that cannot diffuse, along a direction they can follow (D stays 0 where it is 0)."""
    D, zero, n1, _, w = _zero_case()
    _against_fd(oracle, D, np.where(zero, 0.0, n1) * D, w, 0.0, 1.0, "12x9 with zero cells", zero.ravel())


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES + [(12, 9)])
def test_model_identities(oracle, nx, ny, CL, CR):
    """What needs no reference: S_w D = -g (w^T x is homogeneous of degree 0 in D, its gradient of degree -1: Euler),
    <u, S_w v> = <v, S_w u>, S_2w v = 2 S_w v bit for bit (every term is linear in lambda or dlambda, and doubling is exact), and
    curv the long-double sum of d * hv."""
    D, v, u, w = _case(nx, ny)
    hv, curv = _hvp(oracle, D, v, w, CL, CR)
    hu, curu = _hvp(oracle, D, u, w, CL, CR)
    hD, _ = _hvp(oracle, D, D, w, CL, CR)
    g = _gradient(oracle, D, w, CL, CR)
    rel_D = np.max(np.abs(hD + g)) / np.max(np.abs(g))
    lhs, rhs = float(np.sum(u * hv)), float(np.sum(v * hu))
    rel_s = abs(lhs - rhs) / abs(lhs)
    print(f"field hvp identities {nx}x{ny} walls ({CL}, {CR}): |S D + g| / |g| {rel_D:.3e}; <u, S v> {lhs:.6e} <v, S u> {rhs:.6e} "
          f"rel {rel_s:.3e}; curv {float(curv):.6e} {float(curu):.6e}")
    assert rel_D <= 1e-12, rel_D
    assert rel_s <= 1e-12, (lhs, rhs)
    x, lam, y, m = _planes(oracle, D, v, w, CL, CR)
    h2, c2 = field_hvp(x, 2.0 * lam, y, 2.0 * m, D, v, CL, CR)
    assert np.array_equal(h2, 2.0 * hv) and c2 == 2 * curv
    for c, d, h in ((curv, v, hv), (curu, u, hu)):
        want = np.sum(d.astype(np.longdouble) * h.astype(np.longdouble))
        assert c == want and abs(float(c) - float(np.sum(d * h))) <= 1e-13 * float(np.sum(np.abs(d * h)))


def test_model_zero_diffusivity_cells(oracle):
    """hv = 0 where D == 0, everything is finite, and a non-zero dD on those cells changes no bit -- of the pass on the same
    planes, and of the whole product (both right-hand sides ignore it too)."""
    D, zero, dD, _, w = _zero_case()
    CL, CR = 0.0, 1.0
    fixed = zero.ravel()
    x, lam, y, m = _planes(oracle, D, dD, w, CL, CR, fixed)
    hv, curv = field_hvp(x, lam, y, m, D, dD, CL, CR)
    assert np.all(dD[zero] != 0.0)
    assert np.all(hv[zero] == 0.0)
    assert all(np.all(np.isfinite(a)) for a in (hv, y, m)) and np.isfinite(float(curv))
    assert np.any(hv[~zero] != 0.0)
    hv0, curv0 = field_hvp(x, lam, y, m, D, np.where(zero, 0.0, dD), CL, CR)
    assert np.array_equal(hv0, hv) and curv0 == curv
    hv1, curv1 = _hvp(oracle, D, np.where(zero, 0.0, dD), w, CL, CR, fixed)
    assert np.array_equal(hv1, hv) and curv1 == curv


def _usage(unit):
    out, cur = {}, None
    for line in remarks_of(unit).splitlines():
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            cur = out.setdefault(mm.group(1), {})
            continue
        mm = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|"
                       r"VGPRs Spill|SGPRs Spill): (\d+)", line)
        if mm and cur is not None:
            cur[mm.group(1).split(" [")[0]] = int(mm.group(2))
    return out


def test_fhvp_kernels_resources():
    """k_fhvp (kernels_facepass.hpp with FieldHvpPass, five planes besides D): nothing spilled, no AGPRs, at most 168 VGPRs --
    three waves per SIMD -- and no LDS; k_pass_final, the final kernel it launches, uses the 16 wave sums of its reduction, 128 bytes, and no scratch.  And
    k_hvp keeps its four waves: the walk was not changed for it."""
    seen = set()
    for name, u in _usage("api_facepass").items():
        if "6k_fhvpE" in name:
            seen.add("k_fhvp")
            print(f"k_fhvp: {u}")
            assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["VGPRs"] <= 168 and u["AGPRs"] == 0, (name, u)
            assert u["LDS Size"] == 0 and u["Occupancy"] >= 3, (name, u)
        if "12k_pass_finalE" in name:
            seen.add("k_pass_final")
            assert u["ScratchSize"] == 0 and u["LDS Size"] == 128, (name, u)
    assert seen == {"k_fhvp", "k_pass_final"}
    hvp = [u for name, u in _usage("api_facepass").items() if "5k_hvpE" in name]
    assert len(hvp) == 1
    assert hvp[0]["VGPRs"] <= 128 and hvp[0]["Occupancy"] >= 4 and hvp[0]["ScratchSize"] == 0, hvp[0]
