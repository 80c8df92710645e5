"""Conjugate-gradient solver (deff_solve_cg), host side: the references the GPU tests compare with -- the direct
block-tridiagonal solve (checked here against numpy's dense solve), the 5-point operator and a plain Jacobi-preconditioned
CG in numpy at any precision (checked against the dense solve and against itself in long double) -- the library's export,
and the CG kernels' register / scratch budget on the ISA hipcc emits for gfx950.  No GPU needed."""
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


def apply_A(A, X, nx, ny):
    """A X of the 5-point operator (A[n][5] = P, W, E, S(row+1), N(row-1); links beyond the walls and the first / last row
    dropped) as (ny, nx), in the dtype numpy promotes A and X to."""
    X = np.asarray(X).reshape(ny, nx)
    A = np.asarray(A).reshape(ny, nx, 5)
    Ax = A[..., 0] * X
    Ax[:, 1:] += A[:, 1:, 1] * X[:, :-1]
    Ax[:, :-1] += A[:, :-1, 2] * X[:, 1:]
    Ax[:-1, :] += A[:-1, :, 3] * X[1:, :]
    Ax[1:, :] += A[1:, :, 4] * X[:-1, :]
    return Ax


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b * b)))


def residual_np(A, b, x, nx, ny):
    """||b - A x|| / ||b|| with numpy, in the dtype of its arguments (inf for b = 0 and r != 0, 0 for both 0)."""
    r = np.asarray(b).reshape(ny, nx) - apply_A(A, x, nx, ny)
    rr, bb = np.sum(r * r), np.sum(np.asarray(b) ** 2)
    if bb == 0:
        return 0.0 if rr == 0 else float("inf")
    return float(np.sqrt(rr) / np.sqrt(bb))


def decoupled_of(A, b):
    """Rows the library takes out of the system: four zero links and b = 0."""
    return np.all(np.asarray(A)[:, 1:] == 0.0, axis=1) & (np.asarray(b) == 0.0)


class PCGTrace:
    """What pcg_numpy returns: fields[k] = x after k iterations (the requested counts it reached, and the last one), `iters`
    where it stopped, `rel_rec` = ||r|| / ||b|| of the recurrence's r there and `rel_true` = ||b - A x|| / ||b||."""
    __slots__ = ("fields", "iters", "rel_rec", "rel_true", "x")


def pcg_numpy(A, b, x0, nx, ny, iters, dtype, rtol=None):
    """Textbook Jacobi-preconditioned conjugate gradients on the 5-point system, every array and sum in `dtype`, with the
    library's conventions: decoupled rows hold x = p = r = z = 0; z = r * (1 / A0); an image stops at the first iteration
    (0 included) whose recurrence residual has ||r||^2 <= rtol^2 ||b||^2 (rtol None: never), or after max(iters).
    `iters`: an iteration count or several."""
    want = sorted({int(iters)} if np.isscalar(iters) else {int(k) for k in iters})
    A = np.asarray(A, dtype=dtype).reshape(ny, nx, 5)
    b = np.asarray(b, dtype=dtype).reshape(ny, nx)
    act = ~decoupled_of(A.reshape(-1, 5), b.ravel()).reshape(ny, nx)
    minv = np.zeros((ny, nx), dtype=dtype)
    minv[act] = dtype(1) / A[..., 0][act]
    x = np.where(act, np.asarray(x0, dtype=dtype).reshape(ny, nx), dtype(0))
    r = np.where(act, b - apply_A(A, x, nx, ny), dtype(0))
    bb = np.sum(b * b)
    tol2bb = None if rtol is None else dtype(rtol) * dtype(rtol) * bb
    z = r * minv
    p = z.copy()
    rho = np.sum(r * z)
    out = PCGTrace()
    out.fields = {}
    k = 0
    rr = np.sum(r * r)
    while True:
        if k in want:
            out.fields[k] = x.copy()
        if (tol2bb is not None and rr <= tol2bb) or k >= want[-1]:
            break
        q = np.where(act, apply_A(A, p, nx, ny), dtype(0))
        alpha = rho / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        rr = np.sum(r * r)
        z = r * minv
        rho_new = np.sum(r * z)
        p = z + (rho_new / rho) * p
        rho = rho_new
    out.fields[k] = x.copy()
    out.x = x
    out.iters = k
    with np.errstate(divide="ignore", invalid="ignore"):
        out.rel_rec = float(np.sqrt(rr) / np.sqrt(bb)) if bb > 0 else (0.0 if rr == 0 else float("inf"))
    rt = np.where(act, b - apply_A(A, x, nx, ny), dtype(0))
    rrt = np.sum(rt * rt)
    out.rel_true = float(np.sqrt(rrt) / np.sqrt(bb)) if bb > 0 else (0.0 if rrt == 0 else float("inf"))
    return out


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


@pytest.mark.parametrize("nx,ny,seed", [(5, 4, 0), (7, 6, 1), (4, 9, 2), (12, 3, 3), (1, 5, 4), (6, 1, 5)])
def test_pcg_numpy_matches_dense_solve(nx, ny, seed):
    rng = np.random.default_rng(seed)
    A, b = random_spd_5pt(rng, nx, ny)
    want = np.linalg.solve(dense_of(A, nx, ny), b).reshape(ny, nx)
    x0 = rng.standard_normal((ny, nx))
    assert np.allclose(apply_A(A, x0, nx, ny).ravel(), dense_of(A, nx, ny) @ x0.ravel(), rtol=1e-13, atol=1e-13)
    t = pcg_numpy(A, b, x0, nx, ny, 10 * nx * ny, np.float64, rtol=1e-12)
    assert t.iters <= nx * ny + 5 and t.rel_rec <= 1e-12 and t.rel_true <= 1e-11, (t.iters, t.rel_rec, t.rel_true)
    assert rel_l2(t.x, want) <= 1e-9, rel_l2(t.x, want)


def test_pcg_numpy_keeps_decoupled_rows_at_zero():
    rng = np.random.default_rng(11)
    nx, ny = 7, 6
    A, b = random_spd_5pt(rng, nx, ny)
    A = A.reshape(ny, nx, 5)
    # cut cell (2, 3) out: its row and every link into it are zero
    A[2, 3] = 0.0
    A[2, 4, 1] = A[2, 2, 2] = A[1, 3, 3] = A[3, 3, 4] = 0.0
    A = A.reshape(-1, 5)
    b[2 * nx + 3] = 0.0
    dec = decoupled_of(A, b)
    assert dec.sum() == 1
    t = pcg_numpy(A, b, np.ones((ny, nx)), nx, ny, 500, np.float64, rtol=1e-12)
    want = block_thomas(A, b, nx, ny, dec)
    assert t.x[2, 3] == 0.0 and all(f[2, 3] == 0.0 for f in t.fields.values())
    assert rel_l2(t.x, want) <= 1e-9


def synth_system(ob, nx, ny, Ds=1e-3, Df=1.0, CL=0.0, CR=1.0, seed=12345, img=0):
    pix = ob.synth_mask(nx, ny, seed, img)
    D = ob.fill_D_2phase(pix, Df, Ds)
    A, b = ob.discretize(D, CL, CR)
    return pix, D, A, b


K_PARITY = (1, 2, 3, 5, 10, 20)


def test_pcg_numpy_float64_against_longdouble(oracle):
    """g(k): the rel-L2 gap between the float64 and the long double trajectory after k iterations -- the reference's own
    spread, from which the GPU's iteration-parity bar is built (test_gpu_cg.py)."""
    nx, ny = 40, 32
    _, _, A, b = synth_system(oracle, nx, ny)
    x0 = oracle.linear_guess(nx, ny, 0.0, 1.0)
    t64 = pcg_numpy(A, b, x0, nx, ny, K_PARITY, np.float64)
    tld = pcg_numpy(A, b, x0, nx, ny, K_PARITY, np.longdouble)
    for k in K_PARITY:
        g = rel_l2(t64.fields[k], tld.fields[k])
        print(f"g({k}) = {g:.3e}")
        assert np.isfinite(g) and g < 1e-9, (k, g)


def test_float64_residual_evaluation_error(oracle):
    """The additive 1e-13 of the GPU tests' residual bar: ||b - A x|| / ||b|| of a converged field evaluated in float64 is
    off from the long double evaluation by the rounding of b - A x, at most about eps || |A| |x| || / ||b||.  With x in
    [0, 1] and b on the wall columns only that model is 2.2e-15 at 130 x 71 and grows like sqrt(nx): 1.2e-14 at 4096
    columns, a factor 8 below the 1e-13."""
    nx, ny = 130, 71
    _, _, A, b = synth_system(oracle, nx, ny)
    t = pcg_numpy(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), nx, ny, 100000, np.float64, rtol=1e-13)
    ld = np.longdouble
    e64, eld = residual_np(A, b, t.x, nx, ny), residual_np(A.astype(ld), b.astype(ld), t.x.astype(ld), nx, ny)
    model = np.finfo(np.float64).eps * np.linalg.norm(apply_A(np.abs(A), np.abs(t.x), nx, ny)) / np.linalg.norm(b)
    print(f"float64 {e64:.3e}  long double {eld:.3e}  model {model:.3e}")
    assert abs(e64 - eld) <= model <= 1e-14
    assert model * np.sqrt(4096 / nx) <= 2e-14


# (nx, ny, Ds, rtol) of the case the GPU test of the restart rounds runs (test_gpu_cg.py::test_cg_restart_rounds)
RESTART_CASE = (130, 71, 1e-6, 1e-14)


def test_restart_case_drifts_in_the_reference(oracle):
    """Contrast 1e6 at rtol 1e-14: the recurrence's residual reaches the threshold (about 23 000 iterations) while b - A x of
    the same field is still several times above it (measured: 9.9e-15 against 4.0e-14) -- a CG that trusts the recurrence
    would call this converged."""
    nx, ny, Ds, rtol = RESTART_CASE
    _, _, A, b = synth_system(oracle, nx, ny, Ds=Ds)
    t = pcg_numpy(A, b, oracle.linear_guess(nx, ny, 0.0, 1.0), nx, ny, 300000, np.float64, rtol=rtol)
    print(t.iters, t.rel_rec, t.rel_true)
    assert t.iters < 300000 and t.rel_rec <= rtol
    assert t.rel_true > 2 * rtol, (t.rel_rec, t.rel_true)
