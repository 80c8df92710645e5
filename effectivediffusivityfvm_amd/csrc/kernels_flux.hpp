// kernels_flux.hpp -- the flux field: the flux through every face of the current field and the total flux through every
// vertical section, in one streaming pass over x and D (gfx950, wave64, FP64; the reference has the two wall columns only,
// cuh:1256-1257).  k_flux is the pass, k_flux_sections adds the work items' column sums.  Launched from api_flux.hip.
//
// These doubles, in this order (tests/flux_model.py states them in numpy; the library is built without contraction).  dx, dy
// are deff_mesh's, whm is fvm_row.hpp's, row 0 is the top row and "S" is row + 1, as in fvm_row().  For cell p with east
// neighbour e and south neighbour s:
//   interior E face   ke = whm(dx / 2, dx / 2, Dp, De);   fx[p] = ((ke * dy) / dx) * (xe - xp)
//   right wall        fx[p] = ((Dp * dy) / (dx / 2)) * (CR - xp)                  (the last column)
//   left wall         left[row] = ((Dp * dy) / (dx / 2)) * (xp - CL)              (column 0)
//   interior S face   ks = whm(dy / 2, dy / 2, Ds, Dp);   fy[p] = ((ks * dx) / dy) * (xs - xp)
//   an image's last row   fy[p] = +0.0: nothing crosses between the images of a stack.
// These are the conductances of fvm_row() in its operation order, so with fxW[p] the east flux of the west neighbour (or
// left) and fyN[p] the south flux of the north neighbour (or 0), fxW - fx + fyN - fy at cell p is (A x - b)[p] up to rounding.
// The sign is the reference's Residual(): "higher index minus lower"; the physical flux is its negative.
// WEIGHTS: Residual() (cuh:479-485) weights vertical faces with dy / dx; the assembly weights them with dx / dy.  This pass
// follows the ASSEMBLY, so the identity above also holds on meshes whose cells are not square.
// D == 0 needs no special case: whm's quotient w / 0 is +inf, its result 0, and the flux 0.
//
// Sections: per image W + 1 of them (W the mesh width): Q[0] = sum over rows of left, Q[j] = sum over rows of fx[row, j - 1],
// Q[W] the right wall.  ORDER of a section's sum: the rows of an image are cut into runs of 8 * kt rows (the work items);
// within a run a column's terms are added top to bottom, starting from the first; the runs are added in order, starting from
// the first run.  Every column belongs to one lane: no cross-lane reduction, the same bits on every call.
//
// Divisions: whm(w, w, p, q) = (w + w) / (w / p + w / q).  A cell's quotients w / D are computed once -- dx / 2 over D in the
// row in hand, dy / 2 over D for the row below, which keeps it when it becomes the row in hand: four divisions per lane and
// row -- and a face then costs two more, the harmonic mean's and the one by dx (dy): twelve per lane and row for four faces.
// Byte model: x, D read and fx, fy written, 32 B per cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_reduce.hpp"
#include "kernels_facepass.hpp"                  // fp_readlane, FP_ROWS, FP_COLS, FpTag

namespace deff {

struct FluxGeom {
    double dx, dy, hx, hy;                       // hx = dx / 2, hy = dy / 2
};

// what a lane holds of one row: two cells (.x = a, .y = b) of the field and of D
struct FluxRow { double2 x, D; };

// ((whm(w, w, Dp, Dq) * m) / d) * (xq - xp) from the cells' quotients qp = w / Dp, qq = w / Dq and w2 = w + w
__device__ __forceinline__ double flux_face(double w2, double qp, double qq, double m, double d, double xp, double xq)
{
    const double k = w2 / (qp + qq);
    return ((k * m) / d) * (xq - xp);
}

// The body of a __global__ __launch_bounds__(256) kernel.  One wave per work item of cell_pass_items = `kt` consecutive tiles
// of FP_ROWS rows x 128 columns of one image, 4 work items per workgroup; a lane holds two cells (a, b) of each row.
//  - Rows of x and D pass through a window of three (the row in hand, the one below it for the S faces, the one in flight):
//    the 16-byte loads of row r + 2 are issued before the arithmetic of row r.  Rows are clamped into the image, never tested,
//    and every lane loads (a lane beyond the arrays reads the row's first cells).
//  - Every face is evaluated once: per row a lane computes a|b, b|the next lane's a (wave_shl:1 of x and of the quotient
//    dx / 2 over D) and its two S faces.  A cell stores its E and its S face; nothing is carried from the row above.
//  - Lane 63's east neighbour is the cell east of the strip: per tile, lanes 0...7 load it for one row each, a tile ahead,
//    and a row takes it with v_readlane as the `old` operand of the lane shift.
//  - Only the last strip (EDGE) knows the right wall, the cells beyond the mesh and the pad column, by per-lane selects.
//  - Strip 0 also evaluates the left wall: lane 0 writes left[row] and adds it up.
// colpart[(img * cpi + chunk) * nx + col] = the item's sum of fx down column col, wallpart[img * cpi + chunk] that of left.
// Addresses are 64-bit.  No LDS, no atomics, no waiting.
__device__ __forceinline__ void flux_pass(const double *__restrict__ x, const double *__restrict__ D, int nx, int nxt, int ny,
                                          int nimg, int ntx, int cpi, int kt, FluxGeom g, double CL, double CR,
                                          double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ left,
                                          double *__restrict__ colpart, double *__restrict__ wallpart)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t gy = (size_t)nimg * (size_t)cpi;
    const size_t wt = (size_t)blockIdx.x * 4u + (size_t)wave;
    if (wt >= (size_t)ntx * gy) return;
    const int tx = (int)(wt / gy);
    const size_t ty = wt % gy;
    const int img = (int)(ty / (size_t)cpi), chunk = (int)(ty - (size_t)img * (size_t)cpi);
    const int l_begin = chunk * FP_ROWS * kt;                    // rows [l_begin, l_end) of the image
    const int l_end = min(l_begin + FP_ROWS * kt, ny);
    const int col0 = tx * FP_COLS, col = col0 + 2 * lane;
    const size_t ibase = (size_t)img * (size_t)ny * (size_t)nx;
    const double *xi = x + ibase, *Di = D + ibase;
    double *fxi = fx + ibase, *fyi = fy + ibase;
    const double wx2 = g.hx + g.hx, wy2 = g.hy + g.hy;

    auto run = [&](auto edge_tag) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        const bool va = !EDGE || col < nxt, vb = !EDGE || col + 1 < nxt;        // cells of the mesh
        const bool a_last = EDGE && col == nxt - 1, b_last = EDGE && col + 1 == nxt - 1;
        const bool st = !EDGE || col < nx;                                       // lanes inside the arrays
        const int colx = st ? col : 0;
        auto load_row = [&](int li, FluxRow &r) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(li, ny - 1) * (size_t)nx;              // wave-uniform clamp
            r.x = *reinterpret_cast<const double2 *>(xi + rb + colx);
            r.D = *reinterpret_cast<const double2 *>(Di + rb + colx);
        };
        // the cell east of the strip: lane h < 8 holds row l + h of the tile; lanes above 7 repeat lane 7
        const int hq = min(lane, FP_ROWS - 1);
        const int hcol = (!EDGE && col0 + FP_COLS < nxt) ? col0 + FP_COLS : 0;
        struct Outer { double x, D; };
        auto load_outer = [&](int l, Outer &o) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(l + hq, ny - 1) * (size_t)nx;
            o.x = xi[rb + hcol];
            o.D = Di[rb + hcol];
        };

        FluxRow c, n, f;                                         // the row in hand, the next, the one in flight
        Outer o, o2;
        load_row(l_begin, c);
        load_row(l_begin + 1, n);
        load_outer(l_begin, o);
        double qyA = g.hy / c.D.x, qyB = g.hy / c.D.y;           // dy / 2 over D of the row in hand
        double accA = 0.0, accB = 0.0, accW = 0.0;
#pragma unroll 1
        for (int l = l_begin; l < l_end; l += FP_ROWS) {
            load_outer(l + FP_ROWS, o2);
            const double oq = g.hx / o.D;                        // lanes 0...7: dx / 2 over D of the cell east of the strip
#pragma unroll
            for (int q = 0; q < FP_ROWS; ++q) {
                const int r = l + q;
                if (r >= l_end) break;                           // wave-uniform: the item's (or the image's) last rows
                load_row(r + 2, f);
                const double qxA = g.hx / c.D.x, qxB = g.hx / c.D.y;
                const double qnA = g.hy / n.D.x, qnB = g.hy / n.D.y;
                // the next lane's a; lane 63 keeps the cell east of the strip (wave_shl:1)
                const double xE = dpp_f64_keep<0x130>(c.x.x, fp_readlane(o.x, q));
                const double qxE = dpp_f64_keep<0x130>(qxA, fp_readlane(oq, q));
                double fa = flux_face(wx2, qxA, qxB, g.dy, g.dx, c.x.x, c.x.y);      // a | b
                double fb = flux_face(wx2, qxB, qxE, g.dy, g.dx, c.x.y, xE);         // b | the next lane's a
                double sa = flux_face(wy2, qnA, qyA, g.dx, g.dy, c.x.x, n.x.x);      // a | the cell below
                double sb = flux_face(wy2, qnB, qyB, g.dx, g.dy, c.x.y, n.x.y);
                if constexpr (EDGE) {                                // the right wall, the cells beyond it
                    if (a_last) fa = ((c.D.x * g.dy) / g.hx) * (CR - c.x.x);
                    if (b_last) fb = ((c.D.y * g.dy) / g.hx) * (CR - c.x.y);
                    if (!va) { fa = 0.0; sa = 0.0; }
                    if (!vb) { fb = 0.0; sb = 0.0; }
                }
                if (r == ny - 1) { sa = 0.0; sb = 0.0; }             // wave-uniform
                if (tx == 0) {                                       // wave-uniform: the left wall
                    const double wl = ((c.D.x * g.dy) / g.hx) * (c.x.x - CL);
                    accW += wl;
                    if (lane == 0) left[(size_t)img * (size_t)ny + (size_t)r] = wl;
                }
                accA += fa;
                accB += fb;
                if (st) {
                    const size_t at = (size_t)r * (size_t)nx + col;
                    *reinterpret_cast<double2 *>(fxi + at) = make_double2(fa, fb);
                    *reinterpret_cast<double2 *>(fyi + at) = make_double2(sa, sb);
                }
                qyA = qnA; qyB = qnB;
                c = n; n = f;
            }
            o = o2;
        }
        const size_t item = (size_t)img * (size_t)cpi + (size_t)chunk;
        if (st) *reinterpret_cast<double2 *>(colpart + item * (size_t)nx + col) = make_double2(accA, accB);
        if (tx == 0 && lane == 0) wallpart[item] = accW;
    };
    if (tx == ntx - 1) run(FpTag<true>{});
    else run(FpTag<false>{});
}

// The body of a __global__ __launch_bounds__(256) kernel, one thread per (image, section): Q[img * (W + 1) + j] = the `cpi`
// chunk partials of section j in chunk order, starting from the first.
__device__ __forceinline__ void flux_sections_body(const double *__restrict__ colpart, const double *__restrict__ wallpart,
                                                   int nx, int nxt, int nimg, int cpi, double *__restrict__ Q)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)nxt + 1;
    if (t >= per * (size_t)nimg) return;
    const size_t img = t / per, j = t - img * per;
    const double *p = j == 0 ? wallpart + img * (size_t)cpi : colpart + img * (size_t)cpi * (size_t)nx + (j - 1);
    const size_t stride = j == 0 ? 1 : (size_t)nx;
    double s = p[0];
    for (int ch = 1; ch < cpi; ++ch) s += p[(size_t)ch * stride];
    Q[t] = s;
}

}  // namespace deff
