"""The flux field (deff_flux_field_D) in numpy: the normative expressions of include/deff_amd.h, in exactly that operation
order, vectorised, and the section sums in the library's stated order.  Every double is the library's."""
import numpy as np


def whm(w1, w2, x1, x2):
    """WeightedHarmonicMean, cuh:347-360 (fvm_row.hpp): x == 0 gives w / 0 = +inf and H = 0."""
    with np.errstate(divide="ignore"):
        return (w1 + w2) / (w1 / x1 + w2 / x2)


def flux_field(x, D, CL, CR):
    """x, D: (ny, nx) float64 of ONE image.  Returns (fx, fy, left): the flux through the E face of every cell (the right wall's
    in the last column), through its S face (row + 1; +0.0 in the last row), and through the left wall per row."""
    x = np.asarray(x, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    ny, nx = x.shape
    dx, dy = 1.0 / nx, 1.0 / ny
    fx = np.zeros((ny, nx))
    fy = np.zeros((ny, nx))
    ke = whm(dx / 2, dx / 2, D[:, :-1], D[:, 1:])
    fx[:, :-1] = ((ke * dy) / dx) * (x[:, 1:] - x[:, :-1])
    fx[:, -1] = ((D[:, -1] * dy) / (dx / 2)) * (CR - x[:, -1])
    left = ((D[:, 0] * dy) / (dx / 2)) * (x[:, 0] - CL)
    ks = whm(dy / 2, dy / 2, D[1:, :], D[:-1, :])
    fy[:-1, :] = ((ks * dx) / dy) * (x[1:, :] - x[:-1, :])
    return fx, fy, left


def divergence(fx, fy, left):
    """fxW - fx + fyN - fy per cell: (A x - b)[p] up to rounding."""
    ny, nx = fx.shape
    fxW = np.concatenate([left[:, None], fx[:, :-1]], axis=1)
    fyN = np.concatenate([np.zeros((1, nx)), fy[:-1, :]], axis=0)
    return ((fxW - fx) + fyN) - fy


def _ordered(col, ny, kt):
    """Sum of col[0:ny] (one column's terms per row; trailing axes are columns): runs of 8 * kt rows, each added top to bottom
    starting from its first term, the runs added in order starting from the first."""
    run = 8 * kt
    total = None
    for lo in range(0, ny, run):
        s = col[lo].copy()
        for r in range(lo + 1, min(lo + run, ny)):
            s = s + col[r]
        total = s if total is None else total + s
    return total


def sections(fx, left, ny, kt):
    """Q[0 ... nx] of one image: Q[0] = sum of left, Q[j] = sum of fx[:, j - 1], in the library's order for runs of kt tiles."""
    assert fx.shape[0] == ny and left.shape == (ny,) and kt >= 1
    return np.concatenate([np.atleast_1d(_ordered(left, ny, kt)), _ordered(fx, ny, kt)])


def flux_vectors(fx, fy, left):
    """Cell-centred physical flux densities: Jx = -(fxW + fx) / (2 dy), Jy = -(fyN + fy) / (2 dx)."""
    ny, nx = fx.shape
    dx, dy = 1.0 / nx, 1.0 / ny
    fxW = np.concatenate([left[:, None], fx[:, :-1]], axis=1)
    fyN = np.concatenate([np.zeros((1, nx)), fy[:-1, :]], axis=0)
    return -(fxW + fx) / (2 * dy), -(fyN + fy) / (2 * dx)
