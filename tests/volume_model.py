"""numpy model of the volume code (fvm_row3 in fvm_row.hpp, kernels_cg_volume.hpp): the 7-point rows of an nx x ny x nz mesh on the
unit cube in fvm_row3's operation order, the same operator as a dense matrix, and a textbook Jacobi-preconditioned CG with the
library's decoupled-cell rule.  Arrays are (nz, ny, nx); A is (n, 7) = P, W, E, S(row+1), N(row-1), B(slice-1), F(slice+1)."""
import numpy as np

P, W, E, S, N, B, F = range(7)


def whm(w1, w2, x1, x2):
    """WeightedHarmonicMean: x == 0 gives w/0 = inf and a mean of 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w1 + w2) / (w1 / x1 + w2 / x2)


def _shift(D, axis, step):
    """D of the neighbour at index + step along axis, clamped at the ends (the clamped values are never used)."""
    idx = np.clip(np.arange(D.shape[axis]) + step, 0, D.shape[axis] - 1)
    return np.take(D, idx, axis=axis)


def rows3(D, CL, CR):
    """(A (n, 7), b (n,)) of the D volume, every expression in fvm_row3's order, float64."""
    D = np.asarray(D, dtype=np.float64)
    nz, ny, nx = D.shape
    dx, dy, dz = 1.0 / nx, 1.0 / ny, 1.0 / nz
    Dw, De = _shift(D, 2, -1), _shift(D, 2, 1)
    Dn, Ds = _shift(D, 1, -1), _shift(D, 1, 1)
    Db, Df = _shift(D, 0, -1), _shift(D, 0, 1)
    j = np.arange(nx)[None, None, :]
    i = np.arange(ny)[None, :, None]
    k = np.arange(nz)[:, None, None]
    zero = np.zeros_like(D)
    # x block
    kw = whm(dx / 2, dx / 2, D, Dw)
    ke = whm(dx / 2, dx / 2, D, De)
    first, last = j == 0, j == nx - 1
    lw, le = kw * dy * dz / dx, ke * dy * dz / dx                  # interior-face terms
    ww = D * dy * dz / (dx / 2)                                    # wall term: kw = Dp (first) / ke = Dp (last), dxw = dx / 2
    aW = np.where(first, zero, -kw * dy * dz / dx)
    aE = np.where(last, zero, -ke * dy * dz / dx)
    a0 = np.where(first, le + ww, np.where(last, ww + lw, le + lw))
    b = np.where(first, CL * D * dy * dz / (dx / 2), np.where(last, CR * D * dy * dz / (dx / 2), zero))
    # y block
    ks = whm(dy / 2, dy / 2, Ds, D)
    kn = whm(dy / 2, dy / 2, D, Dn)
    first, last = i == 0, i == ny - 1
    ts, tn = ks * dx * dz / dy, kn * dx * dz / dy
    aS = np.where(last, zero, -ks * dx * dz / dy)
    aN = np.where(first, zero, -kn * dx * dz / dy)
    a0 = a0 + np.where(first, ts, np.where(last, tn, tn + ts))
    # z block
    aB, aF = zero.copy(), zero.copy()
    if nz > 1:
        kb = whm(dz / 2, dz / 2, D, Db)
        kf = whm(dz / 2, dz / 2, Df, D)
        first, last = k == 0, k == nz - 1
        tb, tf = kb * dx * dy / dz, kf * dx * dy / dz
        aB = np.where(first, zero, -kb * dx * dy / dz)
        aF = np.where(last, zero, -kf * dx * dy / dz)
        a0 = a0 + np.where(first, tf, np.where(last, tb, tb + tf))
    A = np.stack([a0, aW, aE, aS, aN, aB, aF], axis=-1).reshape(-1, 7)
    return A, b.reshape(-1)


def apply3(A, X, shape):
    """A X of the 7-point operator as (nz, ny, nx) (links out of the volume, and N / S links out of a slice, dropped), in the
    dtype numpy promotes A and X to."""
    nz, ny, nx = shape
    X = np.asarray(X).reshape(nz, ny, nx)
    A = np.asarray(A).reshape(nz, ny, nx, 7)
    Ax = A[..., P] * X
    Ax[:, :, 1:] += A[:, :, 1:, W] * X[:, :, :-1]
    Ax[:, :, :-1] += A[:, :, :-1, E] * X[:, :, 1:]
    Ax[:, :-1, :] += A[:, :-1, :, S] * X[:, 1:, :]
    Ax[:, 1:, :] += A[:, 1:, :, N] * X[:, :-1, :]
    Ax[1:] += A[1:, ..., B] * X[:-1]
    Ax[:-1] += A[:-1, ..., F] * X[1:]
    return Ax


def dense3(A, shape):
    """The same operator as a dense (n, n) matrix."""
    nz, ny, nx = shape
    n = nx * ny * nz
    A = np.asarray(A).reshape(n, 7)
    M = np.zeros((n, n))
    p = np.arange(n)
    j, i, k = p % nx, (p // nx) % ny, p // (nx * ny)
    M[p, p] = A[:, P]
    for col, ok, off in ((W, j > 0, -1), (E, j < nx - 1, 1), (S, i < ny - 1, nx), (N, i > 0, -nx), (B, k > 0, -nx * ny),
                         (F, k < nz - 1, nx * ny)):
        M[p[ok], p[ok] + off] = A[ok, col]
    return M


def decoupled3(A, b):
    """Rows the library takes out of the system: six zero links and b = 0."""
    return np.all(np.asarray(A)[:, 1:] == 0.0, axis=1) & (np.asarray(b) == 0.0)


def residual3(A, b, x, shape, dtype=np.float64):
    """||b - A x|| / ||b|| in dtype, x read as 0 on decoupled cells (inf for b = 0 and r != 0, 0 for both 0)."""
    A, b = np.asarray(A, dtype=dtype), np.asarray(b, dtype=dtype)
    x = np.where(decoupled3(A, b).reshape(shape), dtype(0), np.asarray(x, dtype=dtype).reshape(shape))
    r = b.reshape(shape) - apply3(A, x, shape)
    rr, bb = np.sum(r * r), np.sum(b * b)
    if bb == 0:
        return 0.0 if rr == 0 else float("inf")
    return float(np.sqrt(rr) / np.sqrt(bb))


def pcg(A, b, x0, shape, iters, dtype, rtol=None):
    """Textbook Jacobi-preconditioned CG on the 7-point system, every array and sum in `dtype`, with the library's
    conventions: decoupled rows hold x = p = r = z = 0; z = r * (1 / A0); the iteration stops at the first iteration (0
    included) whose recurrence residual has ||r||^2 <= rtol^2 ||b||^2 (rtol None: never), or after max(iters).
    Returns ({k: x after k iterations, for the requested counts reached and the last}, iterations done)."""
    want = sorted({int(iters)} if np.isscalar(iters) else {int(k) for k in iters})
    A = np.asarray(A, dtype=dtype)
    b = np.asarray(b, dtype=dtype).reshape(shape)
    act = ~decoupled3(A, b.ravel()).reshape(shape)
    minv = np.zeros(shape, dtype=dtype)
    minv[act] = dtype(1) / A[:, P].reshape(shape)[act]
    x = np.where(act, np.asarray(x0, dtype=dtype).reshape(shape), dtype(0))
    r = np.where(act, b - apply3(A, x, shape), dtype(0))
    bb = np.sum(b * b)
    tol2bb = None if rtol is None else dtype(rtol) * dtype(rtol) * bb
    z = r * minv
    p = z.copy()
    rho = np.sum(r * z)
    fields = {}
    k = 0
    rr = np.sum(r * r)
    while True:
        if k in want:
            fields[k] = x.copy()
        if (tol2bb is not None and rr <= tol2bb) or k >= want[-1]:
            break
        q = np.where(act, apply3(A, p, shape), dtype(0))
        alpha = rho / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        rr = np.sum(r * r)
        z = r * minv
        rho_new = np.sum(r * z)
        p = z + (rho_new / rho) * p
        rho = rho_new
    fields[k] = x.copy()
    return fields, k


def deff_of(x, D, CL, CR):
    """The library's Deff of a field: the mean wall flux density over all ny * nz rows and both walls, / (CR - CL)."""
    x = np.asarray(x, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    nz, ny, nx = D.shape
    dx = 1.0 / nx
    L = D[..., 0] * (x[..., 0] - CL) / (dx / 2.0)
    R = D[..., -1] * (CR - x[..., -1]) / (dx / 2.0)
    return float((L.sum() + R.sum()) / (2.0 * ny * nz) / (CR - CL))


def seeded_D(nx, ny, nz, seed=None):
    """The tests' D volume: uniform in [1e-3, 2] with 10 % exact zeros."""
    rng = np.random.default_rng(1000003 * nx + 1009 * ny + nz if seed is None else seed)
    D = rng.uniform(1e-3, 2.0, (nz, ny, nx))
    D[rng.random((nz, ny, nx)) < 0.10] = 0.0
    return D


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
