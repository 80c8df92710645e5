/* prescaled_model.c -- CPU model of the pre-scaled five-FMA Jacobi sweep (deff_set_tuning(ctx, "prescaled", 1)): the
 * definition the tests hold the library to, bit for bit.  Built by tests/test_prescaled_model.py as a shared object with
 * -ffp-contract=off; every fused operation below is an explicit, correctly rounded fma() (libm's, or the hardware
 * instruction where the build enables it) -- never a * b + c.
 *
 * System: the oracle's A[n][5] = (A0, aW, aE, aS, aN) and b[n], row-major nx x ny mesh, S = the row below (p + nx).
 *   c0 = w / A0;  aK' = c0 * aK (K = W, E, S, N);  b' = c0 * b        -- one rounded product each, once per row
 *   acc = fma(1 - w, xC, b'); acc = fma(-aW', xW, acc); acc = fma(-aE', xE, acc); acc = fma(-aS', xS, acc);
 *   xNew = fma(-aN', xN, acc)
 * Every term is always evaluated; a neighbour outside the mesh reads as +0.0. */
#include <math.h>
#include <stddef.h>
#include <string.h>

/* Ap[n][4] = (aW', aE', aS', aN'), bp[n] */
void prescaled_table(const double *A, const double *b, long n, double w, double *Ap, double *bp)
{
    for (long p = 0; p < n; p++) {
        const double c0 = w / A[p * 5 + 0];
        for (int k = 0; k < 4; k++) Ap[p * 4 + k] = c0 * A[p * 5 + 1 + k];
        bp[p] = c0 * b[p];
    }
}

static void sweep(const double *Ap, const double *bp, const double *x, double *xn, int nx, int ny, double omw)
{
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t p = (size_t)j * nx + i;
            const double xw = i > 0 ? x[p - 1] : 0.0;
            const double xe = i < nx - 1 ? x[p + 1] : 0.0;
            const double xs = j < ny - 1 ? x[p + nx] : 0.0;
            const double xnn = j > 0 ? x[p - nx] : 0.0;
            double acc = fma(omw, x[p], bp[p]);
            acc = fma(-Ap[p * 4 + 0], xw, acc);
            acc = fma(-Ap[p * 4 + 1], xe, acc);
            acc = fma(-Ap[p * 4 + 2], xs, acc);
            xn[p] = fma(-Ap[p * 4 + 3], xnn, acc);
        }
}

/* nsweeps sweeps; x is the field in and out, tmp a scratch field of the same size */
void prescaled_sweeps(const double *Ap, const double *bp, double *x, double *tmp, int nx, int ny, long nsweeps, double w)
{
    const double omw = 1.0 - w;
    double *cur = x, *nxt = tmp;
    for (long k = 0; k < nsweeps; k++) {
        sweep(Ap, bp, cur, nxt, nx, ny, omw);
        double *t = cur; cur = nxt; nxt = t;
    }
    if (cur != x) memcpy(x, cur, sizeof(double) * (size_t)nx * ny);
}
