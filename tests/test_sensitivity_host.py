"""The Deff gradient (deff_sensitivity / deff_sensitivity_D), host side: the library's exports, the numpy model of the
normative expressions (tests/sensitivity_model.py) against central finite differences of the wall-flux Deff of a direct solve,
Euler's identity, cells that cannot diffuse, and the kernels' register / scratch / LDS budget on the ISA hipcc emits for
gfx950.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sensitivity_model import sensitivity
from test_cg_host import block_thomas

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_sensitivity_D", "deff_sensitivity", "deff_device_sensitivity")
SHAPES = [(5, 7), (6, 4), (12, 9)]                       # nx, ny: non-square cells
WALLS = [(0.0, 1.0), (2.0, -1.0)]


def test_library_exports_sensitivity():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("sens_kt", "sens_items"):
        assert f'"{key}"' in header, key
    assert callable(pkg.Solver.sensitivity) and callable(pkg.Solver.device_sensitivity_ptr)
    # argument checks come before any device work
    assert L.deff_sensitivity_D(None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_sensitivity(None, None, None, None) == -1
    assert L.deff_device_sensitivity(None, None, None) == -1


def _solve(oracle, D, CL, CR):
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    return block_thomas(A, b, nx, ny)


def _deff(oracle, D, CL, CR):
    return oracle.flux_deff(_solve(oracle, D, CL, CR), D, CL, CR)[0]


def _central_fd(oracle, D, CL, CR, h):
    fd = np.zeros_like(D)
    for p in np.ndindex(*D.shape):
        Dp, Dm = D.copy(), D.copy()
        Dp[p] = D[p] * (1.0 + h)
        Dm[p] = D[p] * (1.0 - h)
        fd[p] = (_deff(oracle, Dp, CL, CR) - _deff(oracle, Dm, CL, CR)) / (Dp[p] - Dm[p])
    return fd


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_against_finite_differences(oracle, nx, ny, CL, CR):
    """The model's map on the direct solve's field against central differences of the wall-flux Deff.  Bar: 10 x the gap
    between the differences at relative steps 1e-5 and 1e-6 -- the finite differences' own uncertainty (DESIGN.md lists
    the gaps measured)."""
    rng = np.random.default_rng(1000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    g, _ = sensitivity(_solve(oracle, D, CL, CR), D, CL, CR)
    fd5 = _central_fd(oracle, D, CL, CR, 1e-5)
    fd6 = _central_fd(oracle, D, CL, CR, 1e-6)
    scale = np.max(np.abs(g))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(g - fd5)) / scale
    print(f"sensitivity fd {nx}x{ny} walls ({CL}, {CR}): gap {gap:.3e} err {err:.3e}")
    # the differences themselves are usable: a wrong term or weight shifts entries by O(1) of the largest one, so a bar of
    # 10 x gap <= 1e-3 still tells.  (Round-off of a difference: the direct solve's error in Deff, ~1e-12 at these condition
    # numbers, over the step h D[p] with D[p] down to e^-5: up to ~1e-5 of the largest entry.)
    assert gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_euler_sum_is_deff(oracle, nx, ny, CL, CR):
    """Deff is homogeneous of degree 1 in D: sum of D * g equals the direct solve's wall-flux Deff."""
    rng = np.random.default_rng(1000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    x = _solve(oracle, D, CL, CR)
    _, euler = sensitivity(x, D, CL, CR)
    deff = oracle.flux_deff(x, D, CL, CR)[0]
    rel = abs(float(euler) - deff) / abs(deff)
    print(f"sensitivity euler {nx}x{ny} walls ({CL}, {CR}): rel {rel:.3e}")
    assert rel <= 1e-13, (float(euler), deff)


def test_model_zero_diffusivity_cells(oracle):
    """Cells with D == 0 hold CG's x = 0 and get g = 0; their neighbours' terms towards them are 0, everything is finite."""
    nx, ny = 7, 6
    rng = np.random.default_rng(5)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    zero = np.zeros((ny, nx), dtype=bool)
    zero[1, 2] = zero[1, 3] = zero[4, 0] = zero[3, 6] = zero[5, 5] = True
    D[zero] = 0.0
    A, b = oracle.discretize(D, 0.0, 1.0)
    x = block_thomas(A, b, nx, ny, fixed=zero.ravel())
    g, euler = sensitivity(x, D, 0.0, 1.0)
    assert np.all(g[zero] == 0.0)
    assert np.all(np.isfinite(g)) and np.isfinite(float(euler))
    assert np.all(g[~zero] >= 0.0) and np.any(g[~zero] > 0.0)
    deff = oracle.flux_deff(x, D, 0.0, 1.0)[0]
    assert abs(float(euler) - deff) <= 1e-12 * abs(deff)


def test_sensitivity_kernels_resources():
    """k_sens (kernels_sens.hpp) spills nothing, keeps to 128 VGPRs (four waves per SIMD: a streaming kernel needs its loads
    in flight) and uses no LDS; k_pass_final, the final kernel it launches, uses the 16 wave sums of its reduction, 128 bytes."""
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
        if "6k_sensE" in name:
            seen.add("k_sens")
            assert u["ScratchSize"] == 0 and u["VGPRs"] <= 128 and u["AGPRs"] == 0, (name, u)
            assert u["LDS"] == 0 and u["Occupancy"] >= 4, (name, u)
        if "12k_pass_finalE" in name:
            seen.add("k_pass_final")
            assert u["ScratchSize"] == 0 and u["LDS"] <= 128, (name, u)
    assert seen == {"k_sens", "k_pass_final"}
