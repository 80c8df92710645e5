"""Volumes on the host: the exports, the numpy model of fvm_row3 (volume_model.py) against the oracle's 2-D assembly at nz = 1,
its symmetry and row sums, the physics of the system it builds (dense solves) and the build figures of the four new kernels."""
import os
import re

import numpy as np
import pytest

import volume_model as vm
from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
NEW_SYMBOLS = ("deff_volume_create", "deff_volume_destroy", "deff_volume_mesh", "deff_volume_assemble_from_D",
               "deff_volume_get_system", "deff_volume_init_linear", "deff_volume_set_field", "deff_volume_get_field",
               "deff_volume_device_field", "deff_volume_flux", "deff_volume_solve_cg", "deff_volume_get_plan")
CL, CR = 0.25, 1.5
U = 2.0 ** -53


def test_library_exports_volumes():
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/deff_amd.h"
        assert name in _capi.SYMBOLS and hasattr(L, name), name
    for m in ("assemble_from_D", "get_system", "init_linear", "set_field", "get_field", "flux", "solve_cg", "plan_value", "close"):
        assert callable(getattr(pkg.Volume, m)), m
    # argument checks come before any device work
    assert L.deff_volume_create(0, 4, 4, 2, None) == -1
    assert L.deff_volume_assemble_from_D(None, np.zeros(4), 0.0, 1.0) == -1
    assert L.deff_volume_solve_cg(None, 1e-10, 10, 1, None, None, None) == -1
    assert L.deff_volume_get_plan(None, b"cg_kr", None) == -1
    assert L.deff_volume_destroy(None) == 0


@pytest.mark.parametrize("nx,ny", [(2, 2), (9, 7), (33, 40)])
def test_model_of_one_slice_is_the_oracles_2d_assembly(oracle, nx, ny):
    D = vm.seeded_D(nx, ny, 1)
    assert (D == 0.0).any() or nx * ny < 10
    A3, b3 = vm.rows3(D, CL, CR)
    A2, b2 = oracle.discretize(D[0], CL, CR)
    assert vm.same_bits(A3[:, :5], A2) and vm.same_bits(b3, b2)
    assert np.all(A3[:, 5:] == 0.0)


@pytest.mark.parametrize("nx,ny,nz", [(2, 2, 2), (9, 7, 3), (5, 4, 6), (16, 3, 5)])
def test_model_links_are_symmetric_and_rows_sum(nx, ny, nz):
    D = vm.seeded_D(nx, ny, nz)
    A, b = vm.rows3(D, CL, CR)
    A = A.reshape(nz, ny, nx, 7)
    assert vm.same_bits(A[:, :, :-1, vm.E], A[:, :, 1:, vm.W])
    assert vm.same_bits(A[:, :-1, :, vm.S], A[:, 1:, :, vm.N])
    assert vm.same_bits(A[:-1, ..., vm.F], A[1:, ..., vm.B])
    # nothing links out of the volume
    assert np.all(A[:, :, 0, vm.W] == 0) and np.all(A[:, :, -1, vm.E] == 0) and np.all(A[:, 0, :, vm.N] == 0)
    assert np.all(A[:, -1, :, vm.S] == 0) and np.all(A[0, ..., vm.B] == 0) and np.all(A[-1, ..., vm.F] == 0)
    # a0 = -(sum of the links) + the wall term, to one rounding per term: the seven terms are the same doubles on both sides
    # (a link is the negated term, exactly), all of one sign, and each side adds them in its own order with at most seven
    # roundings of at most 2^-53 relative each -- 14 in all
    dx, dy, dz = 1.0 / nx, 1.0 / ny, 1.0 / nz
    wall = np.zeros((nz, ny, nx))
    wall[:, :, 0] = D[:, :, 0] * dy * dz / (dx / 2)
    wall[:, :, -1] = D[:, :, -1] * dy * dz / (dx / 2)
    want = -A[..., 1:].sum(axis=-1) + wall
    assert np.all(np.abs(A[..., 0] - want) <= 14 * U * np.abs(want))
    # and b is the wall term times the wall value
    bw = np.zeros((nz, ny, nx))
    bw[:, :, 0], bw[:, :, -1] = CL * wall[:, :, 0], CR * wall[:, :, -1]
    assert np.all(np.abs(b.reshape(nz, ny, nx) - bw) <= 8 * U * np.abs(bw))


def solve_dense(D, cl=CL, cr=CR):
    """(field, Deff, bar) of the model's system by numpy's dense solve; bar = 64 * 2^-53 * cond(A) of that case."""
    nz, ny, nx = D.shape
    A, b = vm.rows3(D, cl, cr)
    M = vm.dense3(A, D.shape)
    assert np.array_equal(M, M.T)
    x = np.linalg.solve(M, b).reshape(D.shape)
    return x, vm.deff_of(x, D, cl, cr), 64 * U * np.linalg.cond(M)


SHAPES = [(6, 5, 4), (9, 4, 3), (4, 7, 5)]


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_homogeneous_volume_has_the_linear_field(nx, ny, nz):
    D0 = 0.75
    x, deff, bar = solve_dense(np.full((nz, ny, nx), D0))
    want = CL + (CR - CL) * (np.arange(nx) + 0.5) / nx
    assert np.max(np.abs(x - want[None, None, :])) <= bar * np.max(np.abs(want))
    assert abs(deff - D0) <= bar * D0


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_layers_in_series_give_the_harmonic_mean(nx, ny, nz):
    rng = np.random.default_rng(nx)
    d = rng.uniform(0.2, 2.0, nx)
    x, deff, bar = solve_dense(np.broadcast_to(d[None, None, :], (nz, ny, nx)).copy())
    want = nx / np.sum(1.0 / d)
    assert abs(deff - want) <= bar * want
    assert np.max(np.abs(x - x[:1, :1, :])) <= bar * np.max(np.abs(x))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_layers_in_parallel_give_the_arithmetic_mean(nx, ny, nz, axis):
    rng = np.random.default_rng(ny + 10 * axis)
    d = rng.uniform(0.2, 2.0, (nz, ny)[axis])
    D = np.empty((nz, ny, nx))
    D[...] = d[:, None, None] if axis == 0 else d[None, :, None]
    x, deff, bar = solve_dense(D)
    assert abs(deff - d.mean()) <= bar * d.mean()
    want = CL + (CR - CL) * (np.arange(nx) + 0.5) / nx
    assert np.max(np.abs(x - want[None, None, :])) <= bar * np.max(np.abs(want))


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
def test_z_uniform_volume_is_the_2d_problem_in_every_slice(oracle, nx, ny, nz):
    rng = np.random.default_rng(7 * nx + ny)
    D2 = rng.uniform(0.05, 2.0, (ny, nx))
    x3, deff3, bar3 = solve_dense(np.broadcast_to(D2[None], (nz, ny, nx)).copy())
    x2, deff2, bar2 = solve_dense(D2[None])
    # the one-slice model is the oracle's 2-D system (above): this is the 2-D field and the 2-D Deff
    A2, b2 = oracle.discretize(D2, CL, CR)
    assert vm.same_bits(vm.rows3(D2[None], CL, CR)[0][:, :5], A2)
    bar = bar3 + bar2
    assert np.max(np.abs(x3 - x2)) <= bar * np.max(np.abs(x2))
    assert abs(deff3 - deff2) <= bar * abs(deff2)


def test_model_pcg_converges_to_the_dense_solve():
    D = vm.seeded_D(9, 7, 3)
    A, b = vm.rows3(D, CL, CR)
    shape = D.shape
    dec = vm.decoupled3(A, b)
    assert dec.any() and not dec.all()
    M = vm.dense3(A, shape)[np.ix_(~dec, ~dec)]
    want = np.zeros(dec.size)
    want[~dec] = np.linalg.solve(M, b[~dec])
    x0 = np.broadcast_to((np.arange(9) / 9 * (CR - CL) + CL)[None, None, :], shape)
    fields, k = vm.pcg(A, b, x0, shape, 10_000, np.float64, rtol=1e-13)
    assert k < 10_000
    x = fields[k].ravel()
    assert np.all(x[dec] == 0.0)
    assert np.linalg.norm(x - want) <= 64 * U * np.linalg.cond(M) * np.linalg.norm(want)
    assert vm.residual3(A, b, x, shape) <= 2e-13


def test_volume_kernel_resources():
    """The four kernels of kernels_cg_volume.hpp: nothing spilled, no LDS."""
    path = os.path.join(CSRC, "build", "api_cg.usage.txt")
    assert os.path.exists(path), "build/api_cg.usage.txt missing"
    usage, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    names = {"24k_assemble_volume_from_DE": "k_assemble_volume_from_D", "13k_cgv_prepareE": "k_cgv_prepare", "9k_cgv_dirE": "k_cgv_dir",
             "11k_cgv_residE": "k_cgv_resid"}
    seen = set()
    for name, u in usage.items():
        for mangled, plain in names.items():
            if mangled in name:
                seen.add(plain)
                print(f"{plain}: {u}")
                assert u["ScratchSize"] == 0 and u["LDS"] == 0, (name, u)
    assert seen == set(names.values()), seen
