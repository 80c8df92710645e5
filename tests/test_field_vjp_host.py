"""The field adjoint (deff_solve_adjoint, deff_field_vjp_D), host side: the library's exports, the numpy model of the normative
expressions (tests/field_vjp_model.py) against central finite differences of sum(w * x(D)) on direct solves, the Euler sum
(0 for a converged field, whatever lambda is), cells that cannot diffuse, and the kernels' register / scratch / LDS budget on
the ISA hipcc emits for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from field_vjp_model import field_vjp
from test_cg_host import block_thomas

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_solve_adjoint", "deff_set_adjoint", "deff_get_adjoint", "deff_device_adjoint", "deff_field_vjp_D",
               "deff_device_field_vjp")
SHAPES = [(5, 7), (6, 4), (12, 9)]                       # nx, ny: non-square cells
WALLS = [(0.0, 1.0), (2.0, -1.0)]


def test_library_exports_field_vjp():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("vjp_kt", "vjp_items"):
        assert f'"{key}"' in header, key
    for m in ("solve_adjoint", "set_adjoint", "get_adjoint", "device_adjoint_ptr", "field_vjp", "device_field_vjp_ptr"):
        assert callable(getattr(pkg.Solver, m)), m
    assert callable(pkg.concentration_field)
    # argument checks come before any device work
    assert L.deff_solve_adjoint(None, None, 1e-10, 10, 1, None) == -1
    assert L.deff_set_adjoint(None, None) == -1
    assert L.deff_get_adjoint(None, None) == -1
    assert L.deff_device_adjoint(None, None, None) == -1
    assert L.deff_field_vjp_D(None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_device_field_vjp(None, None, None) == -1


def _case(nx, ny):
    rng = np.random.default_rng(1000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    w = rng.standard_normal((ny, nx))
    return D, w


def _solve(oracle, D, CL, CR):
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    return A, block_thomas(A, b, nx, ny)


def _loss(oracle, D, w, CL, CR):
    return float(np.sum(w * _solve(oracle, D, CL, CR)[1]))


def central_fd(loss, D, h):
    """Central differences of loss(D) per cell at the relative step h."""
    fd = np.zeros_like(D)
    for p in np.ndindex(*D.shape):
        Dp, Dm = D.copy(), D.copy()
        Dp[p] = D[p] * (1.0 + h)
        Dm[p] = D[p] * (1.0 - h)
        fd[p] = (loss(Dp) - loss(Dm)) / (Dp[p] - Dm[p])
    return fd


def _model(oracle, D, w, CL, CR):
    ny, nx = D.shape
    A, x = _solve(oracle, D, CL, CR)
    lam = block_thomas(A, w.ravel(), nx, ny)
    return field_vjp(x, lam, D, CL, CR)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_against_finite_differences(oracle, nx, ny, CL, CR):
    """The model's map on the direct solves x = A^-1 b, lambda = A^-1 w against central differences of sum(w * x(D)).  Bar:
    10 x the gap between the differences at relative steps 1e-5 and 1e-6 -- the finite differences' own uncertainty, the rule
    of test_sensitivity_host.py for the Deff gradient."""
    D, w = _case(nx, ny)
    g, _ = _model(oracle, D, w, CL, CR)
    fd5 = central_fd(lambda Dq: _loss(oracle, Dq, w, CL, CR), D, 1e-5)
    fd6 = central_fd(lambda Dq: _loss(oracle, Dq, w, CL, CR), D, 1e-6)
    scale = np.max(np.abs(g))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(g - fd5)) / scale
    print(f"field vjp fd {nx}x{ny} walls ({CL}, {CR}): gap {gap:.3e} err {err:.3e}")
    # a wrong term, weight or sign shifts entries by O(1) of the largest one: the differences must be usable for the bar to tell
    assert gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_euler_sum_is_zero(oracle, nx, ny, CL, CR):
    """A and b are homogeneous of degree 1 in D, x of degree 0: sum of D * g = -lambda^T (A x - b) = 0 for the direct solve's x."""
    D, w = _case(nx, ny)
    g, euler = _model(oracle, D, w, CL, CR)
    size = float(np.sum(np.abs(D * g)))
    print(f"field vjp euler {nx}x{ny} walls ({CL}, {CR}): |sum| / sum|.| {abs(float(euler)) / size:.3e}")
    assert abs(float(euler)) <= 1e-12 * size, (float(euler), size)


def test_model_zero_diffusivity_cells(oracle):
    """Cells with D == 0 -- on a wall, next to each other -- and a wall cell cut off by them: g = 0 where D == 0, the terms of
    the neighbours towards them are 0, everything is finite."""
    nx, ny = 7, 6
    rng = np.random.default_rng(5)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    w = rng.standard_normal((ny, nx))
    zero = np.zeros((ny, nx), dtype=bool)
    zero[1, 2] = zero[1, 3] = zero[4, 0] = zero[3, 6] = True
    zero[5, 5] = zero[4, 6] = True                        # (5, 6), on the right wall, keeps no interior face
    D[zero] = 0.0
    A, b = oracle.discretize(D, 0.0, 1.0)
    assert np.all(A[5 * nx + 6, 1:] == 0.0) and A[5 * nx + 6, 0] > 0.0
    x = block_thomas(A, b, nx, ny, fixed=zero.ravel())
    lam = block_thomas(A, w.ravel(), nx, ny, fixed=zero.ravel())
    g, euler = field_vjp(x, lam, D, 0.0, 1.0)
    assert np.all(g[zero] == 0.0)
    assert np.all(np.isfinite(g)) and np.isfinite(float(euler))
    assert np.any(g[~zero] != 0.0)
    assert abs(float(euler)) <= 1e-12 * float(np.sum(np.abs(D * g)))


def test_field_vjp_kernels_resources():
    """k_vjp (kernels_vjp.hpp) under k_sens's bars: nothing spilled, at most 128 VGPRs (four waves per SIMD: a streaming kernel
    needs its loads in flight), no LDS; k_pass_final, the final kernel it launches, uses the 16 wave sums of its reduction, 128 bytes."""
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
        if "5k_vjpE" in name:
            seen.add("k_vjp")
            print(f"k_vjp: {u}")
            assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128 and u["AGPRs"] == 0, (name, u)
            assert u["LDS"] == 0 and u["Occupancy"] >= 4, (name, u)
        if "12k_pass_finalE" in name:
            seen.add("k_pass_final")
            assert u["ScratchSize"] == 0 and u["LDS"] <= 128, (name, u)
    assert seen == {"k_vjp", "k_pass_final"}
