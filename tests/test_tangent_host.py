"""The field tangent (deff_tangent_rhs_D, deff_solve_tangent), host side: the library's exports, the numpy model of the normative
expressions (tests/tangent_model.py) against central finite differences of the direct solve x(D) along a direction, the
direction D (the pass returns the forward residual), the dot-product identity with the field adjoint's model, cells that cannot
diffuse, and the kernels' register / scratch / LDS budget on the ISA hipcc emits for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from field_vjp_model import field_vjp
from tangent_model import tangent_rhs
from test_cg_host import block_thomas

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_tangent_rhs_D", "deff_device_tangent_rhs", "deff_solve_tangent", "deff_get_tangent", "deff_device_tangent")
SHAPES = [(5, 7), (6, 4), (12, 9)]                       # nx, ny: non-square cells
WALLS = [(0.0, 1.0), (2.0, -1.0)]


def test_library_exports_tangent():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("tan_kt", "tan_items"):
        assert f'"{key}"' in header, key
    for m in ("tangent_rhs", "solve_tangent", "get_tangent", "device_tangent_ptr", "device_tangent_rhs_ptr", "field_jvp"):
        assert callable(getattr(pkg.Solver, m)), m
    # argument checks come before any device work
    assert L.deff_tangent_rhs_D(None, None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_device_tangent_rhs(None, None, None) == -1
    assert L.deff_solve_tangent(None, 1e-10, 10, 1, None) == -1
    assert L.deff_get_tangent(None, None) == -1
    assert L.deff_device_tangent(None, None, None) == -1


def _case(nx, ny):
    rng = np.random.default_rng(1000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    dD = D * rng.standard_normal((ny, nx))               # a direction of D's own size per cell
    w = rng.standard_normal((ny, nx))
    return D, dD, w


def _solve(oracle, D, CL, CR):
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    return A, b, block_thomas(A, b, nx, ny)


def _tangent(oracle, D, dD, CL, CR):
    """The model's dx on direct solves: x = A^-1 b, r from the pass's expressions, dx = A^-1 r."""
    ny, nx = D.shape
    A, b, x = _solve(oracle, D, CL, CR)
    r, norm2 = tangent_rhs(x, D, dD, CL, CR)
    return A, b, x, r, norm2, block_thomas(A, r.ravel(), nx, ny)


def directional_fd(oracle, D, dD, CL, CR, h):
    """Central difference of the direct solve x(D) along dD at the step h."""
    xp = _solve(oracle, D + h * dD, CL, CR)[2]
    xm = _solve(oracle, D - h * dD, CL, CR)[2]
    return (xp - xm) / (2.0 * h)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_against_finite_differences(oracle, nx, ny, CL, CR):
    """dx = block_thomas(A, r) against central differences of x(D +- h dD).  Bar: 10 x the gap between the differences at the
    steps 1e-5 and 1e-6 -- the finite differences' own uncertainty, the rule of test_field_vjp_host.py."""
    D, dD, _ = _case(nx, ny)
    dx = _tangent(oracle, D, dD, CL, CR)[5]
    fd5 = directional_fd(oracle, D, dD, CL, CR, 1e-5)
    fd6 = directional_fd(oracle, D, dD, CL, CR, 1e-6)
    scale = np.max(np.abs(dx))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(dx - fd5)) / scale
    print(f"tangent fd {nx}x{ny} walls ({CL}, {CR}): gap {gap:.3e} err {err:.3e}")
    # a wrong term, weight or sign shifts entries by O(1) of the largest one: the differences must be usable for the bar to tell
    assert scale > 0.0 and gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_direction_D_is_the_forward_residual(oracle, nx, ny, CL, CR):
    """A and b are homogeneous of degree 1 in D: along dD = D, dA = A and db = b, so r = b - A x, 0 for the direct solve's x."""
    D, _, _ = _case(nx, ny)
    A, b, x, r, norm2, _ = _tangent(oracle, D, D, CL, CR)
    rel = float(np.sqrt(norm2)) / float(np.sqrt(np.sum(b * b)))
    print(f"tangent direction D {nx}x{ny} walls ({CL}, {CR}): ||r|| / ||b|| {rel:.3e}")
    assert rel <= 1e-12, rel


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_dot_product_with_the_field_adjoint(oracle, nx, ny, CL, CR):
    """<w, J d> = <J^T w, d>: the tangent's dx against the field adjoint's map on the same direct solves."""
    D, dD, w = _case(nx, ny)
    A, b, x, r, _, dx = _tangent(oracle, D, dD, CL, CR)
    lam = block_thomas(A, w.ravel(), nx, ny)
    g, _ = field_vjp(x, lam, D, CL, CR)
    lhs, rhs = float(np.sum(w * dx)), float(np.sum(g * dD))
    rel = abs(lhs - rhs) / abs(lhs)
    print(f"tangent dot product {nx}x{ny} walls ({CL}, {CR}): <w, dx> {lhs:.6e} <g, d> {rhs:.6e} rel {rel:.3e}")
    assert rel <= 1e-12, (lhs, rhs)


def test_model_zero_diffusivity_cells(oracle):
    """The D == 0 case of test_field_vjp_host.py -- cells on a wall, next to each other, a wall cell cut off by them: r = 0
    where D == 0, everything is finite, and a non-zero dD on those cells changes nothing."""
    nx, ny = 7, 6
    rng = np.random.default_rng(5)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    dD = rng.standard_normal((ny, nx))
    zero = np.zeros((ny, nx), dtype=bool)
    zero[1, 2] = zero[1, 3] = zero[4, 0] = zero[3, 6] = True
    zero[5, 5] = zero[4, 6] = True                        # (5, 6), on the right wall, keeps no interior face
    D[zero] = 0.0
    A, b = oracle.discretize(D, 0.0, 1.0)
    x = block_thomas(A, b, nx, ny, fixed=zero.ravel())
    r, norm2 = tangent_rhs(x, D, dD, 0.0, 1.0)
    assert np.all(dD[zero] != 0.0)
    assert np.all(r[zero] == 0.0)
    assert np.all(np.isfinite(r)) and np.isfinite(float(norm2))
    assert np.any(r[~zero] != 0.0)
    dx = block_thomas(A, r.ravel(), nx, ny, fixed=zero.ravel())
    assert np.all(np.isfinite(dx)) and np.all(dx[zero] == 0.0)
    r0, norm20 = tangent_rhs(x, D, np.where(zero, 0.0, dD), 0.0, 1.0)
    assert np.array_equal(r0, r) and norm20 == norm2
    # and the tangent is the derivative there too: central differences along the direction the cells can follow
    d = np.where(zero, 0.0, dD) * D
    rd, _ = tangent_rhs(x, D, d, 0.0, 1.0)
    dxd = block_thomas(A, rd.ravel(), nx, ny, fixed=zero.ravel())

    def fd(h):
        out = []
        for sgn in (1.0, -1.0):
            Aq, bq = oracle.discretize(D + sgn * h * d, 0.0, 1.0)
            out.append(block_thomas(Aq, bq, nx, ny, fixed=zero.ravel()))
        return (out[0] - out[1]) / (2.0 * h)

    fd5, fd6 = fd(1e-5), fd(1e-6)
    scale = np.max(np.abs(dxd))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(dxd - fd5)) / scale
    print(f"tangent fd with zero cells: gap {gap:.3e} err {err:.3e}")
    assert gap < 1e-4 and err <= 10.0 * gap, (err, gap)


def test_tangent_kernels_resources():
    """k_tan (kernels_facepass.hpp with TanPass) under k_vjp's bars: nothing spilled, at most 128 VGPRs (four waves per SIMD: a
    streaming kernel needs its loads in flight), no LDS; k_pass_final, the final kernel it launches, uses the 16 wave sums of its reduction, 128 bytes."""
    path = os.path.join(CSRC, "build", "api_facepass.usage.txt")
    assert os.path.exists(path), "build/api_facepass.usage.txt missing: api_facepass.hip is not part of the build"
    usage, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    seen = set()
    for name, u in usage.items():
        if "5k_tanE" in name:
            seen.add("k_tan")
            print(f"k_tan: {u}")
            assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128 and u["AGPRs"] == 0, (name, u)
            assert u["LDS"] == 0 and u["Occupancy"] >= 4, (name, u)
        if "12k_pass_finalE" in name:
            seen.add("k_pass_final")
            assert u["ScratchSize"] == 0 and u["LDS"] <= 128, (name, u)
    assert seen == {"k_tan", "k_pass_final"}
