"""The field adjoint's pass (deff_field_vjp_D) in numpy: the normative expressions of include/deff_amd.h, in exactly that
operation order, vectorised.  Every double of the map is the library's; the Euler sum is added in long double."""
import numpy as np


def _face(Dp, Dq, xp, xq, lp, lq, w):
    """The term of cell p from its interior face to q: s = Dp + Dq; t = (s == 0) ? 0 : Dq / s; e = xp - xq; f = lp - lq;
    c = (2.0 * (t * t)) * (w * (e * f))."""
    s = Dp + Dq
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s == 0, 0.0, Dq / s)
    e = xp - xq
    f = lp - lq
    return (2.0 * (t * t)) * (w * (e * f))


def field_vjp(x, lam, D, CL, CR):
    """x, lam, D: (ny, nx) float64 of ONE image.  Returns (g, euler): g[p] = dL/dD[p] as (ny, nx) float64 for the loss whose
    dL/dx is the right-hand side lam solves, and euler = sum of D * g in np.longdouble."""
    x = np.asarray(x, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    ny, nx = x.shape
    dx, dy = 1.0 / nx, 1.0 / ny
    wx, wy = dy / dx, dx / dy
    ww = dy / (dx / 2.0)
    cW = np.zeros((ny, nx))
    cE = np.zeros((ny, nx))
    cN = np.zeros((ny, nx))
    cS = np.zeros((ny, nx))
    cW[:, 1:] = _face(D[:, 1:], D[:, :-1], x[:, 1:], x[:, :-1], lam[:, 1:], lam[:, :-1], wx)
    cE[:, :-1] = _face(D[:, :-1], D[:, 1:], x[:, :-1], x[:, 1:], lam[:, :-1], lam[:, 1:], wx)
    cN[1:, :] = _face(D[1:, :], D[:-1, :], x[1:, :], x[:-1, :], lam[1:, :], lam[:-1, :], wy)
    cS[:-1, :] = _face(D[:-1, :], D[1:, :], x[:-1, :], x[1:, :], lam[:-1, :], lam[1:, :], wy)
    e = x[:, 0] - CL
    cW[:, 0] = ww * (e * lam[:, 0])
    e = x[:, -1] - CR
    cE[:, -1] = ww * (e * lam[:, -1])
    g = -(((cW + cE) + cN) + cS)
    g = np.where(D == 0, 0.0, g)
    euler = np.sum(D.astype(np.longdouble) * g.astype(np.longdouble))
    return g, euler
