"""The Deff gradient of a volume (deff_volume_sensitivity_D) in numpy: the normative expressions of include/deff_amd.h, in exactly
that operation order, vectorised.  Every double of the map is the library's; the Euler sum is added in long double.  With
nz = 1 the weights carry a factor 1.0 and the two absent z terms add +0.0: the bits of sensitivity_model.sensitivity."""
import numpy as np

from sensitivity_model import _face


def sensitivity3(x, D, CL, CR):
    """x, D: (nz, ny, nx) float64.  Returns (g, euler): g[p] = d deff_raw / d D[p] as (nz, ny, nx) float64, and
    euler = sum of D * g in np.longdouble."""
    x = np.asarray(x, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    nz, ny, nx = x.shape
    dx, dy, dz = 1.0 / nx, 1.0 / ny, 1.0 / nz
    wx, wy, wz = dy * dz / dx, dx * dz / dy, dx * dy / dz
    ww = dy * dz / (dx / 2.0)
    cW, cE, cN, cS, cB, cF = (np.zeros((nz, ny, nx)) for _ in range(6))
    cW[:, :, 1:] = _face(D[:, :, 1:], D[:, :, :-1], x[:, :, 1:], x[:, :, :-1], wx)
    cE[:, :, :-1] = _face(D[:, :, :-1], D[:, :, 1:], x[:, :, :-1], x[:, :, 1:], wx)
    cN[:, 1:, :] = _face(D[:, 1:, :], D[:, :-1, :], x[:, 1:, :], x[:, :-1, :], wy)
    cS[:, :-1, :] = _face(D[:, :-1, :], D[:, 1:, :], x[:, :-1, :], x[:, 1:, :], wy)
    cB[1:] = _face(D[1:], D[:-1], x[1:], x[:-1], wz)
    cF[:-1] = _face(D[:-1], D[1:], x[:-1], x[1:], wz)
    e = x[:, :, 0] - CL
    cW[:, :, 0] = ww * (e * e)
    e = x[:, :, -1] - CR
    cE[:, :, -1] = ww * (e * e)
    g = (((((cW + cE) + cN) + cS) + cB) + cF) / ((CR - CL) * (CR - CL))
    g = np.where(D == 0, 0.0, g)
    euler = np.sum(D.astype(np.longdouble) * g.astype(np.longdouble))
    return g, euler
