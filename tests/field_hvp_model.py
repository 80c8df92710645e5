"""The second-order field adjoint's pass (deff_field_vjp_hvp_D) in numpy: the normative expressions of include/deff_amd.h, in
exactly that operation order, vectorised.  Every double of the map is the library's; the curvature is added in long double."""
import numpy as np


def _face(Dp, Dq, dp, dq, xp, xq, lp, lq, yp, yq, mp, mq, w):
    """The term of cell p from its interior face to q: s = Dp + Dq; tq = (s == 0) ? 0 : Dq / s; tp likewise with Dp;
    u = (s == 0) ? 0 : (tp * dq - tq * dp) / s; e = xp - xq; fl = lp - lq; ed = yp - yq; fm = mp - mq; ef = e * fl;
    k = ed * fl + e * fm; c = w * ((4.0 * tq) * (u * ef) + (2.0 * (tq * tq)) * k)."""
    s = Dp + Dq
    with np.errstate(divide="ignore", invalid="ignore"):
        tq = np.where(s == 0, 0.0, Dq / s)
        tp = np.where(s == 0, 0.0, Dp / s)
        u = np.where(s == 0, 0.0, (tp * dq - tq * dp) / s)
    e = xp - xq
    fl = lp - lq
    ed = yp - yq
    fm = mp - mq
    ef = e * fl
    k = ed * fl + e * fm
    return w * ((4.0 * tq) * (u * ef) + (2.0 * (tq * tq)) * k)


def field_hvp(x, lam, y, m, D, dD, CL, CR):
    """x, lam, y, m, D, dD: (ny, nx) float64 of ONE image: the field, lambda (A lambda = w), the field tangent y = dx and
    lambda's tangent m = dlambda along dD.  Returns (hv, curv): hv = S_w dD as (ny, nx) float64, S_w the Hessian of w^T x(D)
    with w fixed, and curv = sum of d * hv in np.longdouble, d = dD where D != 0."""
    x, lam, y, m, D = (np.asarray(a, dtype=np.float64) for a in (x, lam, y, m, D))
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

    def face(p, q, w):
        return _face(D[p], D[q], d[p], d[q], x[p], x[q], lam[p], lam[q], y[p], y[q], m[p], m[q], w)

    cW[R] = face(R, L, wx)
    cE[L] = face(L, R, wx)
    cN[B] = face(B, U, wy)
    cS[U] = face(U, B, wy)
    e = x[:, 0] - CL
    cW[:, 0] = ww * (y[:, 0] * lam[:, 0] + e * m[:, 0])
    e = x[:, -1] - CR
    cE[:, -1] = ww * (y[:, -1] * lam[:, -1] + e * m[:, -1])
    hv = -(((cW + cE) + cN) + cS)
    hv = np.where(D == 0, 0.0, hv)
    curv = np.sum(d.astype(np.longdouble) * hv.astype(np.longdouble))
    return hv, curv
