"""The flux field (deff_flux_field_D, csrc/kernels_flux.hpp), host side: the library's exports, the numpy model of the normative
expressions (tests/flux_model.py) against the assembled system -- the divergence of the face fluxes is A x - b -- and against
the reference's wall fluxes, and the kernel's scratch / LDS budget on the ISA hipcc emits for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import flux_model as fm
from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_flux_field_D", "deff_flux_field", "deff_device_flux_field")
SHAPES = [(2, 2), (9, 7), (17, 13), (24, 31), (40, 33)]     # ny, nx
CL, CR = 0.25, 1.5
U = 2.0 ** -53


def make_case(ny, nx):
    """D in [1e-3, 2] with 10 % of the cells 0, and a random field."""
    rng = np.random.default_rng(1000 * ny + nx)
    D = rng.uniform(1e-3, 2.0, (ny, nx))
    D[rng.random((ny, nx)) < 0.10] = 0.0
    x = rng.uniform(min(CL, CR) - 0.5, max(CL, CR) + 0.5, (ny, nx))
    return x, D


def test_library_exports_flux_field():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for key in ("flux_kt", "flux_items"):
        assert f'"{key}"' in header, key
    for m in ("flux_field", "device_flux_field_ptrs"):
        assert callable(getattr(pkg.Solver, m)), m
    assert callable(pkg.flux_vectors) and pkg.FluxField._fields == ("fx", "fy", "left", "sections")
    # argument checks come before any device work
    assert L.deff_flux_field_D(None, None, 0.0, 1.0, None, None, None, None, None) == -1
    assert L.deff_flux_field(None, None, None, None, None, None) == -1
    assert L.deff_device_flux_field(None, None, None, None) == -1


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_divergence_is_the_assembled_residual(oracle, ny, nx):
    """fxW - fx + fyN - fy = (A x - b)[p] up to rounding, cell by cell: the sum with (b - A x) is within
    8 * 2^-53 * (|A| |x| + |b|).  (A x - b is evaluated in long double: the bound is about the fluxes' roundings.)"""
    x, D = make_case(ny, nx)
    A, b = oracle.discretize(D, CL, CR)
    fx, fy, left = fm.flux_field(x, D, CL, CR)
    assert np.all(np.isfinite(fx)) and np.all(np.isfinite(fy)) and np.all(np.isfinite(left))
    A = A.reshape(ny, nx, 5).astype(np.longdouble)                # P, W, E, S (row + 1), N (row - 1)
    xl = np.pad(x.astype(np.longdouble), 1)
    nb = np.stack([xl[1:-1, 1:-1], xl[1:-1, :-2], xl[1:-1, 2:], xl[2:, 1:-1], xl[:-2, 1:-1]], axis=-1)
    Ax = np.sum(A * nb, axis=-1)
    size = np.sum(np.abs(A) * np.abs(nb), axis=-1) + np.abs(b.reshape(ny, nx))
    off = np.abs(fm.divergence(fx, fy, left).astype(np.longdouble) + (b.reshape(ny, nx) - Ax))
    ratio = float(np.max(off[size > 0] / (8 * U * size[size > 0])))
    print(f"flux divergence {ny}x{nx}: largest |div + (b - A x)| / (8 u (|A||x| + |b|)) = {ratio:.3f}")
    assert np.all(off <= 8 * U * size), ratio
    assert np.any(fy != 0.0) and np.all(fy[-1] == 0.0)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_wall_sections_are_the_references_deff(oracle, ny, nx):
    """(Q[0] + Q[W]) / (2 (CR - CL)) against the reference's flux evaluation (cuh:1256-1263): every term carries at most 3
    roundings and each sum at most ny, so the two agree within 8 ny 2^-53 (sum|left| + sum|fx[:, -1]|) / (2 |CR - CL|)."""
    x, D = make_case(ny, nx)
    fx, fy, left = fm.flux_field(x, D, CL, CR)
    Q = fm.sections(fx, left, ny, 1)
    assert Q.shape == (nx + 1,)
    got = (Q[0] + Q[nx]) / (2 * (CR - CL))
    want = oracle.flux_deff(x, D, CL, CR)[0]
    bar = 8 * ny * U * (np.sum(np.abs(left)) + np.sum(np.abs(fx[:, -1]))) / (2 * abs(CR - CL))
    print(f"flux walls {ny}x{nx}: {got!r} against {want!r}, off by {abs(got - want) / bar:.3f} of the bar")
    assert abs(got - want) <= bar, (got, want, bar)


def test_section_order():
    """sections() adds runs of 8 * kt rows top to bottom and then the runs in order: on terms whose sum depends on the order,
    the stated order's result."""
    ny = 21
    col = np.array([1.0] + [2.0 ** -53] * 20)
    fx = np.stack([col, col[::-1]], axis=1)
    Q = fm.sections(fx, col, ny, 1)
    run0 = 1.0                                                    # 1 + 7 x 2^-53: each addition rounds back to 1
    assert Q[0] == Q[1] == (run0 + 8 * 2.0 ** -53) + 5 * 2.0 ** -53
    assert Q[2] == (8 * 2.0 ** -53 + 8 * 2.0 ** -53) + (4 * 2.0 ** -53 + 1.0)
    assert fm.sections(fx, col, ny, 3)[0] == 1.0                  # one run: every addition rounds back to 1


def test_flux_kernel_resources():
    """k_flux (kernels_flux.hpp): nothing spilled, no LDS."""
    path = os.path.join(CSRC, "build", "api_flux.usage.txt")
    assert os.path.exists(path), "build/api_flux.usage.txt missing: api_flux.hip is not part of the build"
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
        if "6k_fluxE" in name:
            seen.add("k_flux")
            print(f"k_flux: {u}")
            assert u["ScratchSize"] == 0 and u["LDS"] == 0, (name, u)
        if "15k_flux_sectionsE" in name:
            seen.add("k_flux_sections")
            assert u["ScratchSize"] == 0 and u["LDS"] == 0, (name, u)
    assert seen == {"k_flux", "k_flux_sections"}
