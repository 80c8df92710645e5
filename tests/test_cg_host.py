"""Conjugate-gradient solver (deff_solve_cg), host side: the direct block-tridiagonal solve the GPU tests take as their
reference (checked here against numpy's dense solve), the library's export, and the CG kernels' register / scratch budget
on the ISA hipcc emits for gfx950.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")


def block_thomas(A, b, nx, ny, fixed=None):
    """Direct solve of the 5-point system in the reference's AoS layout (A[n][5] = P, W, E, S(row+1), N(row-1), b[n]) by
    block Thomas over the rows (blocks of nx cells: tridiagonal in the row, diagonal couplings to the rows above and below).
    `fixed` (bool, n): cells held at x = 0 -- their rows become identity rows and the links into them are dropped.
    Links beyond the walls (first / last column, first / last row) are ignored.  Returns x as (ny, nx)."""
    A = np.array(A, dtype=np.float64).reshape(ny, nx, 5)
    b = np.array(b, dtype=np.float64).reshape(ny, nx)
    if fixed is not None:
        fx = np.asarray(fixed, dtype=bool).reshape(ny, nx)
        A[fx] = (1.0, 0.0, 0.0, 0.0, 0.0)
        b[fx] = 0.0
        A[:, 1:, 1][fx[:, :-1]] = 0.0                     # W link into a fixed cell
        A[:, :-1, 2][fx[:, 1:]] = 0.0                     # E
        A[:-1, :, 3][fx[1:, :]] = 0.0                     # S (row + 1)
        A[1:, :, 4][fx[:-1, :]] = 0.0                     # N (row - 1)
    cols = np.arange(nx)

    def diag_block(i):
        D = np.zeros((nx, nx))
        D[cols, cols] = A[i, :, 0]
        D[cols[1:], cols[:-1]] = A[i, 1:, 1]
        D[cols[:-1], cols[1:]] = A[i, :-1, 2]
        return D

    Cp = np.zeros((ny, nx, nx))
    dp = np.zeros((ny, nx))
    for i in range(ny):
        M = diag_block(i)
        rhs = b[i].copy()
        if i > 0:
            L = A[i, :, 4]                                  # row i <- row i - 1
            M -= L[:, None] * Cp[i - 1]
            rhs -= L * dp[i - 1]
        U = np.diag(A[i, :, 3]) if i + 1 < ny else np.zeros((nx, nx))
        sol = np.linalg.solve(M, np.column_stack([U, rhs]))
        Cp[i], dp[i] = sol[:, :nx], sol[:, nx]
    x = np.zeros((ny, nx))
    x[ny - 1] = dp[ny - 1]
    for i in range(ny - 2, -1, -1):
        x[i] = dp[i] - Cp[i] @ x[i + 1]
    return x


def dense_of(A, nx, ny):
    """The same operator as a dense matrix (links beyond the walls dropped)."""
    n = nx * ny
    M = np.zeros((n, n))
    for p in range(n):
        i, j = divmod(p, nx)
        M[p, p] = A[p, 0]
        if j > 0: M[p, p - 1] = A[p, 1]
        if j + 1 < nx: M[p, p + 1] = A[p, 2]
        if i + 1 < ny: M[p, p + nx] = A[p, 3]
        if i > 0: M[p, p - nx] = A[p, 4]
    return M


def random_spd_5pt(rng, nx, ny):
    """A symmetric positive definite 5-point system: random face conductances, Dirichlet walls on the left and right."""
    A = np.zeros((ny * nx, 5))
    gh = rng.uniform(1e-3, 1.0, (ny, nx - 1))             # face (i, j) - (i, j + 1)
    gv = rng.uniform(1e-3, 1.0, (ny - 1, nx))             # face (i, j) - (i + 1, j)
    for i in range(ny):
        for j in range(nx):
            p = i * nx + j
            if j > 0: A[p, 1] = -gh[i, j - 1]
            if j + 1 < nx: A[p, 2] = -gh[i, j]
            if i + 1 < ny: A[p, 3] = -gv[i, j]
            if i > 0: A[p, 4] = -gv[i - 1, j]
            A[p, 0] = -A[p, 1:].sum() + (rng.uniform(0.5, 2.0) if j in (0, nx - 1) else 0.0)
    b = rng.standard_normal(ny * nx)
    return A, b


@pytest.mark.parametrize("nx,ny,seed", [(5, 4, 0), (7, 6, 1), (4, 9, 2), (12, 3, 3), (1, 5, 4), (6, 1, 5)])
def test_block_thomas_matches_dense_solve(nx, ny, seed):
    rng = np.random.default_rng(seed)
    A, b = random_spd_5pt(rng, nx, ny)
    M = dense_of(A, nx, ny)
    assert np.allclose(M, M.T)
    want = np.linalg.solve(M, b).reshape(ny, nx)
    got = block_thomas(A, b, nx, ny)
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


def test_block_thomas_fixed_cells():
    """Fixed cells: x = 0 there, and the rest solves the system with those columns dropped."""
    rng = np.random.default_rng(7)
    nx, ny = 6, 5
    A, b = random_spd_5pt(rng, nx, ny)
    fixed = np.zeros(nx * ny, dtype=bool)
    fixed[[8, 9, 20]] = True
    got = block_thomas(A, b, nx, ny, fixed)
    M = dense_of(A, nx, ny)
    keep = ~fixed
    want = np.zeros(nx * ny)
    want[keep] = np.linalg.solve(M[np.ix_(keep, keep)], b[keep])
    assert np.all(got.ravel()[fixed] == 0.0)
    assert np.linalg.norm(got.ravel() - want) <= 1e-12 * np.linalg.norm(want)


def test_library_exports_solve_cg():
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = C.CDLL(lib)
    assert hasattr(L, "deff_solve_cg")
    # argument checks come before any device work
    out = (C.c_byte * 64)()
    assert L.deff_solve_cg(None, C.c_double(1e-10), C.c_int64(10), C.c_int64(1), out, None, None) == -1


def test_cg_kernels_resources():
    """The CG kernels (kernels_cg.hpp) spill nothing.  Streaming kernels (k_cg_dir, k_cg_update, k_cg_resid,
    k_cg_admissible): <= 96 VGPRs, no AGPR, 28.4 KiB of LDS (the 7-plane table) -- 5 waves per SIMD, bounded by the LDS;
    the per-image reductions (k_cg_alpha, k_cg_beta, k_cg_check) <= 32 VGPRs."""
    path = os.path.join(CSRC, "build", "api_cg.usage.txt")
    assert os.path.exists(path), "build/api_cg.usage.txt missing: api_cg.hip is not part of the build"
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
        for k in ("k_cg_dir", "k_cg_update", "k_cg_resid", "k_cg_admissible"):
            if f"{len(k)}{k}" in name:
                seen.add(k)
                assert u["ScratchSize"] == 0 and u["VGPRs"] <= 96 and u["AGPRs"] == 0, (name, u)
                assert u["LDS"] <= 29184 and u["Occupancy"] >= 5, (name, u)
        for k in ("k_cg_alpha", "k_cg_beta", "k_cg_check"):
            if f"{len(k)}{k}" in name:
                seen.add(k)
                assert u["ScratchSize"] == 0 and u["VGPRs"] <= 32, (name, u)
    assert seen == {"k_cg_dir", "k_cg_update", "k_cg_resid", "k_cg_admissible", "k_cg_alpha", "k_cg_beta", "k_cg_check"}
