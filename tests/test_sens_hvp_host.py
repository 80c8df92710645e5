"""The Deff Hessian-vector product (deff_sensitivity_hvp_D, deff_set_tangent), host side: the library's exports, the numpy model
of the normative expressions (tests/sens_hvp_model.py) against central finite differences of the gradient model on direct
solves, the identities that need no reference (H D = 0, symmetry, concavity), cells that cannot diffuse, and the kernels'
register / scratch / LDS budget on the ISA hipcc emits for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sens_hvp_model import sens_hvp
from sensitivity_model import sensitivity
from tangent_model import tangent_rhs
from test_cg_host import block_thomas

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_sensitivity_hvp_D", "deff_device_sensitivity_hvp", "deff_set_tangent")
SHAPES = [(5, 7), (6, 4), (12, 9)]                       # nx, ny: non-square cells
WALLS = [(0.0, 1.0), (2.0, -1.0)]


def test_library_exports_sens_hvp():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("hvp_kt", "hvp_items"):
        assert f'"{key}"' in header, key
    for m in ("sens_hvp", "device_sens_hvp_ptr", "set_tangent", "deff_hvp"):
        assert callable(getattr(pkg.Solver, m)), m
    # argument checks come before any device work
    assert L.deff_sensitivity_hvp_D(None, None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_device_sensitivity_hvp(None, None, None) == -1
    assert L.deff_set_tangent(None, None) == -1


def _case(nx, ny):
    rng = np.random.default_rng(2000 * nx + ny)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    v = D * rng.standard_normal((ny, nx))                # a direction of D's own size per cell
    w = D * rng.standard_normal((ny, nx))
    return D, v, w


def _gradient(oracle, D, CL, CR, fixed=None):
    """The gradient model on the direct solve of D."""
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    return sensitivity(block_thomas(A, b, nx, ny, fixed=fixed), D, CL, CR)[0]


def _hvp(oracle, D, v, CL, CR, fixed=None):
    """The model's H v on direct solves: x = A^-1 b, r from the tangent's expressions, dx = A^-1 r, then the pass."""
    ny, nx = D.shape
    A, b = oracle.discretize(D, CL, CR)
    x = block_thomas(A, b, nx, ny, fixed=fixed)
    r, _ = tangent_rhs(x, D, v, CL, CR)
    y = block_thomas(A, r.ravel(), nx, ny, fixed=fixed)
    return sens_hvp(x, y, D, v, CL, CR) + (x, y)


def _fd(oracle, D, v, CL, CR, h, fixed=None):
    """Central difference of the gradient model on direct solves along v at the step h."""
    return (_gradient(oracle, D + h * v, CL, CR, fixed) - _gradient(oracle, D - h * v, CL, CR, fixed)) / (2.0 * h)


def _against_fd(oracle, D, v, CL, CR, what, fixed=None):
    hv = _hvp(oracle, D, v, CL, CR, fixed)[0]
    fd5, fd6 = _fd(oracle, D, v, CL, CR, 1e-5, fixed), _fd(oracle, D, v, CL, CR, 1e-6, fixed)
    scale = np.max(np.abs(hv))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(hv - fd5)) / scale
    print(f"sens hvp fd {what}: gap {gap:.3e} err {err:.3e}")
    # a wrong term, weight or sign shifts entries by O(1) of the largest one: the differences must be usable for the bar to tell
    assert scale > 0.0 and gap < 1e-4, gap
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_against_finite_differences(oracle, nx, ny, CL, CR):
    """H v against central differences of sensitivity(x(D +- h v), D +- h v).  Bar: 10 x the gap between the differences at the
    steps 1e-5 and 1e-6 -- the finite differences' own uncertainty, the rule of test_sensitivity_host.py -- relative to the
    largest entry of H v, and the gap itself below 1e-4."""
    D, v, _ = _case(nx, ny)
    _against_fd(oracle, D, v, CL, CR, f"{nx}x{ny} walls ({CL}, {CR})")


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_identities(oracle, nx, ny, CL, CR):
    """What needs no reference: H D = 0 (Deff is homogeneous of degree 1 in D, its gradient of degree 0), <w, H v> = <v, H w>,
    and v^T H v < 0 (Deff is a minimum over fields of functions linear in D), with curv the sum of d * hv."""
    D, v, w = _case(nx, ny)
    hv, curv, _, _ = _hvp(oracle, D, v, CL, CR)
    hw, curw, _, _ = _hvp(oracle, D, w, CL, CR)
    hD, _, _, _ = _hvp(oracle, D, D, CL, CR)
    rel_D = np.max(np.abs(hD)) / np.max(np.abs(hv))
    lhs, rhs = float(np.sum(w * hv)), float(np.sum(v * hw))
    rel_s = abs(lhs - rhs) / abs(lhs)
    print(f"sens hvp identities {nx}x{ny} walls ({CL}, {CR}): |H D| / |H v| {rel_D:.3e}; <w, H v> {lhs:.6e} <v, H w> {rhs:.6e} "
          f"rel {rel_s:.3e}; curv {float(curv):.6e} {float(curw):.6e}")
    assert rel_D <= 1e-12, rel_D
    assert rel_s <= 1e-12, (lhs, rhs)
    assert curv < 0 and curw < 0
    for c, d, h in ((curv, v, hv), (curw, w, hw)):
        want = np.sum(d.astype(np.longdouble) * h.astype(np.longdouble))
        assert c == want and abs(float(c) - float(np.sum(d * h))) <= 1e-13 * float(np.sum(np.abs(d * h)))


def test_model_zero_diffusivity_cells(oracle):
    """The D == 0 case of test_tangent_host.py -- cells on a wall, next to each other, a wall cell cut off by them: hv = 0
    where D == 0, everything is finite, a non-zero dD on those cells changes no bit, and H v is the derivative there too."""
    nx, ny = 7, 6
    CL, CR = 0.0, 1.0
    rng = np.random.default_rng(5)
    D = np.exp(2.0 * rng.standard_normal((ny, nx)))
    dD = rng.standard_normal((ny, nx))
    zero = np.zeros((ny, nx), dtype=bool)
    zero[1, 2] = zero[1, 3] = zero[4, 0] = zero[3, 6] = True
    zero[5, 5] = zero[4, 6] = True                        # (5, 6), on the right wall, keeps no interior face
    D[zero] = 0.0
    fixed = zero.ravel()
    hv, curv, x, y = _hvp(oracle, D, dD, CL, CR, fixed)
    assert np.all(dD[zero] != 0.0)
    assert np.all(hv[zero] == 0.0)
    assert np.all(np.isfinite(hv)) and np.isfinite(float(curv)) and np.all(np.isfinite(y))
    assert np.any(hv[~zero] != 0.0) and curv < 0
    hv0, curv0 = sens_hvp(x, y, D, np.where(zero, 0.0, dD), CL, CR)
    assert np.array_equal(hv0, hv) and curv0 == curv
    hv1, curv1, _, y1 = _hvp(oracle, D, np.where(zero, 0.0, dD), CL, CR, fixed)
    assert np.array_equal(y1, y) and np.array_equal(hv1, hv) and curv1 == curv
    # central differences along the direction the cells can follow (D stays 0 where it is 0)
    _against_fd(oracle, D, np.where(zero, 0.0, dD) * D, CL, CR, "with zero cells", fixed)


def test_hvp_kernels_resources():
    """k_hvp (kernels_facepass.hpp with HvpPass) under k_tan's bars: nothing spilled, at most 128 VGPRs (four waves per SIMD: a
    streaming kernel needs its loads in flight), no LDS; k_pass_final, the final kernel it launches, uses the 16 wave sums of its reduction, 128 bytes."""
    path = os.path.join(CSRC, "build", "api_facepass.usage.txt")
    assert os.path.exists(path), "build/api_facepass.usage.txt missing: api_facepass.hip is not part of the build"
    usage, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|"
                      r"VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    seen = set()
    for name, u in usage.items():
        if "5k_hvpE" in name:
            seen.add("k_hvp")
            print(f"k_hvp: {u}")
            assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["VGPRs"] <= 128 and u["AGPRs"] == 0, (name, u)
            assert u["LDS Size"] == 0 and u["Occupancy"] >= 4, (name, u)
        if "12k_pass_finalE" in name:
            seen.add("k_pass_final")
            assert u["ScratchSize"] == 0 and u["LDS Size"] == 128, (name, u)
    assert seen == {"k_hvp", "k_pass_final"}
