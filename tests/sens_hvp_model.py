"""The Deff Hessian-vector product's pass (deff_sensitivity_hvp_D) in numpy: the normative expressions of include/deff_amd.h,
in exactly that operation order, vectorised.  Every double of the map is the library's; the curvature is added in long double."""
import numpy as np


def _face(Dp, Dq, dp, dq, xp, xq, yp, yq, w):
    """The term of cell p from its interior face to q: s = Dp + Dq; tq = (s == 0) ? 0 : Dq / s; tp likewise with Dp;
    u = (s == 0) ? 0 : (tp * dq - tq * dp) / s; e = xp - xq; f = yp - yq;
    c = w * ((4.0 * tq) * (u * (e * e)) + (4.0 * (tq * tq)) * (e * f))."""
    s = Dp + Dq
    with np.errstate(divide="ignore", invalid="ignore"):
        tq = np.where(s == 0, 0.0, Dq / s)
        tp = np.where(s == 0, 0.0, Dp / s)
        u = np.where(s == 0, 0.0, (tp * dq - tq * dp) / s)
    e = xp - xq
    f = yp - yq
    return w * ((4.0 * tq) * (u * (e * e)) + (4.0 * (tq * tq)) * (e * f))


def sens_hvp(x, y, D, dD, CL, CR):
    """x, y, D, dD: (ny, nx) float64 of ONE image, y the field tangent dx along dD.  Returns (hv, curv): hv = H dD as (ny, nx)
    float64, H the Hessian of deff_raw with respect to D, and curv = sum of d * hv in np.longdouble, d = dD where D != 0."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
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
    L, R, U, B = np.s_[:, :-1], np.s_[:, 1:], np.s_[:-1, :], np.s_[1:, :]          # the two cells of a W/E face, of a N/S face
    cW[R] = _face(D[R], D[L], d[R], d[L], x[R], x[L], y[R], y[L], wx)
    cE[L] = _face(D[L], D[R], d[L], d[R], x[L], x[R], y[L], y[R], wx)
    cN[B] = _face(D[B], D[U], d[B], d[U], x[B], x[U], y[B], y[U], wy)
    cS[U] = _face(D[U], D[B], d[U], d[B], x[U], x[B], y[U], y[B], wy)
    e = x[:, 0] - CL
    cW[:, 0] = ww * (2.0 * (e * y[:, 0]))
    e = x[:, -1] - CR
    cE[:, -1] = ww * (2.0 * (e * y[:, -1]))
    hv = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL))
    hv = np.where(D == 0, 0.0, hv)
    curv = np.sum(d.astype(np.longdouble) * hv.astype(np.longdouble))
    return hv, curv
