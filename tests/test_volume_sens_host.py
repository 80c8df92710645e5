"""The Deff gradient of a volume (deff_volume_sensitivity_D), host side: the library's exports, the numpy model of the normative
expressions (tests/volume_sens_model.py) against the 2-D model at one slice, against central finite differences of the
wall-flux Deff of dense solves, Euler's identity, a z-uniform volume, and k_sens3's register / scratch / LDS budget on the ISA
hipcc emits for gfx950.  No GPU needed."""
import functools
import os
import re

import numpy as np
import pytest

import volume_model as vm
from conftest import ROOT
from sensitivity_model import sensitivity
from volume_sens_model import sensitivity3

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_volume_sensitivity_D", "deff_volume_device_sensitivity", "deff_volume_set_tuning")
WALLS = [(0.0, 1.0), (2.0, -1.0)]
FD_SHAPES = [(3, 4, 5), (4, 3, 6), (5, 6, 7)]            # nz, ny, nx
EPS = 2.0 ** -53


def test_library_exports_volume_sensitivity():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS + ("deff_volume_get_plan",):
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for fn in ("sensitivity", "set_tuning", "device_sensitivity_ptr"):
        assert callable(getattr(pkg.Volume, fn)), fn
    assert callable(pkg.effective_diffusivity_volume)
    # argument checks come before any device work
    assert L.deff_volume_sensitivity_D(None, None, 0.0, 1.0, None, None, None) == -1
    assert L.deff_volume_device_sensitivity(None, None, None) == -1
    assert L.deff_volume_set_tuning(None, b"sens_kt", 1) == -1


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nx,ny", [(2, 2), (9, 7), (33, 40)])
def test_one_slice_has_the_2d_models_bits(nx, ny, CL, CR):
    """x * 1.0 is exact and a sum of non-negative terms + 0.0 keeps its bits: nz = 1 is sensitivity_model.sensitivity."""
    D = vm.seeded_D(nx, ny, 1)
    assert (D == 0).any() or nx * ny < 8
    x = np.random.default_rng(7 * nx + ny).standard_normal((1, ny, nx))
    g3, e3 = sensitivity3(x, D, CL, CR)
    g2, e2 = sensitivity(x[0], D[0], CL, CR)
    assert g3.shape == (1, ny, nx) and vm.same_bits(g3[0], g2)
    assert e3 == e2 and isinstance(e3, np.longdouble)


@functools.lru_cache(maxsize=None)
def dense_case(nz, ny, nx, CL, CR, zeros=False):
    """(D, x, deff, cond) of a dense solve of the model's rows: D = exp(N(0, 1)), or seeded_D with its zero cells (decoupled
    rows hold x = 0).  Computed once, never written."""
    if zeros:
        D = vm.seeded_D(nx, ny, nz)
    else:
        D = np.exp(np.random.default_rng(10000 * nz + 100 * ny + nx).standard_normal((nz, ny, nx)))
    x, cond = _solve(D, CL, CR)
    for a in (D, x):
        a.setflags(write=False)
    return D, x, vm.deff_of(x, D, CL, CR), cond


def _solve(D, CL, CR):
    A, b = vm.rows3(D, CL, CR)
    dec = vm.decoupled3(A, b)
    M = vm.dense3(A, D.shape)[np.ix_(~dec, ~dec)]
    x = np.zeros(dec.size)
    x[~dec] = np.linalg.solve(M, b[~dec])
    return x.reshape(D.shape), float(np.linalg.cond(M))


def _central_fd(D, CL, CR, h):
    fd = np.zeros_like(D)
    for p in np.ndindex(*D.shape):
        Dp, Dm = D.copy(), D.copy()
        Dp[p] = D[p] * (1.0 + h)
        Dm[p] = D[p] * (1.0 - h)
        fd[p] = (vm.deff_of(_solve(Dp, CL, CR)[0], Dp, CL, CR) - vm.deff_of(_solve(Dm, CL, CR)[0], Dm, CL, CR)) / (Dp[p] - Dm[p])
    return fd


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nz,ny,nx", FD_SHAPES)
def test_model_against_finite_differences(nz, ny, nx, CL, CR):
    """The model's map on the dense solve's field against central differences of volume_model.deff_of.  Bar: 10 x the gap
    between the differences at relative steps 1e-5 and 1e-6, relative to the map's largest entry -- the finite differences' own
    uncertainty, the rule of test_sensitivity_host.py."""
    D, x, _, _ = dense_case(nz, ny, nx, CL, CR)
    g, _ = sensitivity3(x, D, CL, CR)
    fd5 = _central_fd(D, CL, CR, 1e-5)
    fd6 = _central_fd(D, CL, CR, 1e-6)
    scale = np.max(np.abs(g))
    gap = np.max(np.abs(fd5 - fd6)) / scale
    err = np.max(np.abs(g - fd5)) / scale
    print(f"volume sensitivity fd ({nz},{ny},{nx}) walls ({CL}, {CR}): gap {gap:.3e} err {err:.3e} err/gap {err / gap:.2f}")
    assert gap < 1e-4, gap                     # the differences themselves are usable: a wrong term shifts entries by O(1)
    assert err <= 10.0 * gap, (err, gap)


@pytest.mark.parametrize("CL,CR", WALLS)
@pytest.mark.parametrize("nz,ny,nx,zeros", [s + (False,) for s in FD_SHAPES] + [(3, 5, 6, True), (4, 4, 4, True)])
def test_model_euler_sum_is_deff(nz, ny, nx, zeros, CL, CR):
    """Deff is homogeneous of degree 1 in D: sum of D * g equals the dense solve's wall-flux Deff, within what the solve's
    backward error can move the field by: 64 * 2^-53 * cond(A)."""
    D, x, deff, cond = dense_case(nz, ny, nx, CL, CR, zeros)
    assert (D == 0).any() == zeros
    g, euler = sensitivity3(x, D, CL, CR)
    assert np.all(g[D == 0] == 0.0) and np.all(np.isfinite(g)) and np.all(g >= 0.0)
    rel = abs(float(euler) - deff) / abs(deff)
    print(f"volume sensitivity euler ({nz},{ny},{nx}) zeros={zeros} walls ({CL}, {CR}): rel {rel:.3e} cond {cond:.3e}")
    assert rel <= 64 * EPS * cond, (float(euler), deff, cond)


@pytest.mark.parametrize("nz", [2, 3, 7])
def test_z_uniform_volume_is_the_2d_map_over_nz(nz):
    """D and the field repeated in every slice: the z differences are exactly 0, the x, y and wall weights carry dz = 1 / nz.
    Not bits: fl(fl(dy * dz) / dx) against fl(dy / dx) / nz differ by up to 4 roundings (dz's own, the two products', the
    quotient's), every term is non-negative so the sums add no cancellation, and the chain from a weight to g[p] has six more
    roundings on either side -- w * (e * e), the product with 2 t^2, three additions, the division -- and the final / nz one:
    at most (4 + 2 * 6 + 1) * 2^-53 < 16 * 2^-53 relative per entry."""
    ny, nx = 9, 7
    D2 = vm.seeded_D(nx, ny, 1)[0]
    x2 = np.random.default_rng(nz).uniform(0.0, 1.0, (ny, nx))
    g2, _ = sensitivity(x2, D2, 0.25, 1.5)
    g3, _ = sensitivity3(np.repeat(x2[None], nz, 0), np.repeat(D2[None], nz, 0), 0.25, 1.5)
    want = g2 / nz
    worst = np.max(np.abs(g3 - want[None]) / np.where(want == 0, 1.0, want)[None])
    print(f"z-uniform nz={nz}: worst {worst / EPS:.2f} x 2^-53")
    assert np.all(g3[:, want == 0] == 0.0)
    assert worst <= 16 * EPS, worst


def test_k_sens3_resources():
    """k_sens3 spills nothing and uses no LDS and no AGPRs; at least three waves per SIMD (DESIGN.md section 18 has the
    figures of the build)."""
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
    mine = [(n, u) for n, u in usage.items() if "7k_sens3E" in n]
    assert len(mine) == 1, list(usage)
    name, u = mine[0]
    print(f"k_sens3: VGPRs {u['VGPRs']}, occupancy {u['Occupancy']} waves/SIMD")
    assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["AGPRs"] == 0, (name, u)
    assert u["Occupancy"] >= 3, (name, u)
