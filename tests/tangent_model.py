"""The field tangent's pass (deff_tangent_rhs_D) in numpy: the normative expressions of include/deff_amd.h, in exactly that
operation order, vectorised.  Every double of the map is the library's; the squared norm is added in long double."""
import numpy as np


def _face(Dp, Dq, dp, dq, xp, xq, w):
    """The term of cell p from its interior face to q: s = Dp + Dq; tq = (s == 0) ? 0 : Dq / s; tp likewise with Dp;
    h = (2.0 * (tq * tq)) * dp + (2.0 * (tp * tp)) * dq; e = xp - xq; c = w * (h * e)."""
    s = Dp + Dq
    with np.errstate(divide="ignore", invalid="ignore"):
        tq = np.where(s == 0, 0.0, Dq / s)
        tp = np.where(s == 0, 0.0, Dp / s)
    h = (2.0 * (tq * tq)) * dp + (2.0 * (tp * tp)) * dq
    e = xp - xq
    return w * (h * e)


def tangent_rhs(x, D, dD, CL, CR):
    """x, D, dD: (ny, nx) float64 of ONE image.  Returns (r, norm2): r = db - dA x along dD as (ny, nx) float64 -- the
    right-hand side of A dx = r --, and norm2 = sum of r * r in np.longdouble."""
    x = np.asarray(x, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    d = np.where(D == 0, 0.0, np.asarray(dD, dtype=np.float64))
    ny, nx = x.shape
    dx, dy = 1.0 / nx, 1.0 / ny
    wx, wy = dy / dx, dx / dy
    ww = dy / (dx / 2.0)
    cW = np.zeros((ny, nx))
    cE = np.zeros((ny, nx))
    cN = np.zeros((ny, nx))
    cS = np.zeros((ny, nx))
    cW[:, 1:] = _face(D[:, 1:], D[:, :-1], d[:, 1:], d[:, :-1], x[:, 1:], x[:, :-1], wx)
    cE[:, :-1] = _face(D[:, :-1], D[:, 1:], d[:, :-1], d[:, 1:], x[:, :-1], x[:, 1:], wx)
    cN[1:, :] = _face(D[1:, :], D[:-1, :], d[1:, :], d[:-1, :], x[1:, :], x[:-1, :], wy)
    cS[:-1, :] = _face(D[:-1, :], D[1:, :], d[:-1, :], d[1:, :], x[:-1, :], x[1:, :], wy)
    cW[:, 0] = ww * (d[:, 0] * (x[:, 0] - CL))
    cE[:, -1] = ww * (d[:, -1] * (x[:, -1] - CR))
    r = -(((cW + cE) + cN) + cS)
    r = np.where(D == 0, 0.0, r)
    rl = r.astype(np.longdouble)
    return r, np.sum(rl * rl)
