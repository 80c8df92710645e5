// kernels_vjp.hpp -- the field adjoint's pass: g[p] = dL/dD[p] from the field x, the adjoint field l (A l = dL/dx) and D, one
// streaming pass over three planes (gfx950, wave64, FP64; nothing like it in the reference).
//
// dL/dD[p] = -l^T (dA/dD[p] x - db/dD[p]), and over faces l^T (A x - b) = sum over faces a_f (x_p - x_q)(l_p - l_q) + sum over
// wall cells c_p (x_p - C_wall) l_p.  The chain rule through the harmonic mean H = 2 Dp Dq / (Dp + Dq) is k_sens's:
// dH / dDp = 2 (Dq / (Dp + Dq))^2.  Per cell p, one term per face (weights as the assembly's, fvm_row.hpp: W / E faces carry
// wx = dy / dx, N / S faces wy = dx / dy, a wall ww = dy / (dx / 2)):
//   interior face to q   s = Dp + Dq;  t = (s == 0) ? 0 : Dq / s;  e = xp - xq;  f = lp - lq;  c = (2.0 * (t * t)) * (w * (e * f))
//   left / right wall    e = xp - CL (CR);  f = lp;  c = ww * (e * f)
//   no face (an image's first and last row)   c = +0.0
//   g[p] = -(((cW + cE) + cN) + cS),  and g[p] = 0 where D[p] == 0.  The pad column of an odd mesh width gets 0.
// e and f both change sign exactly when the face is seen from its other cell, so e * f -- and with it w * (e * f) -- has the same
// value from either side (a zero may differ in sign, which no comparison of doubles sees) and is evaluated ONCE per face, with
// one division per cell and face for t (vjp_face): four FP64 divisions per cell and no final one.
// tests/field_vjp_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
//
// The second output, euler[img] = sum over the image's cells of D[p] * g[p], is -l^T (A x - b): 0 for a converged x whatever l
// is (A and b are homogeneous of degree 1 in D), a check that needs no reference.  ORDER of that sum, as k_sens's: a lane adds
// its cells top to bottom through its work item (first cell of its pair, then the second), the 64 lane sums of a wave are
// combined by wave_reduce.hpp's fixed DPP tree, and k_vjp_final (one workgroup of 16 waves per image) has thread t add the work
// items' sums t, t + 1024, ... in index order, the same tree per wave, and thread 0 the 16 wave sums in wave order.  The order
// depends on the launch geometry only: the same bits on every call.
//
// k_vjp is the structure of k_sens (kernels_sens.hpp) with a third stream; nothing is shared with it but wave_reduce.hpp, so
// k_sens's code and registers are what they were.  Byte model: x, l, D read and g written, 32 B per cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_reduce.hpp"

namespace deff {

constexpr int VJP_ROWS = 8;                      // rows per tile
constexpr int VJP_COLS = 128;                    // columns per strip: 2 per lane
template <bool V> struct VjpTag { static constexpr bool value = V; };

// One interior face between cells p and q, weight w: cp = the term of p, cq = the term of q.
__device__ __forceinline__ void vjp_face(double Dp, double Dq, double xp, double xq, double lp, double lq, double w, double &cp,
                                         double &cq)
{
    const double s = Dp + Dq;
    const double e = xp - xq;
    const double f = lp - lq;
    const double wef = w * (e * f);
    const double tq = (s == 0) ? 0 : Dq / s;
    const double tp = (s == 0) ? 0 : Dp / s;
    cp = (2.0 * (tq * tq)) * wef;
    cq = (2.0 * (tp * tp)) * wef;
}

__device__ __forceinline__ double vjp_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One wave per work item = `kt` consecutive tiles of VJP_ROWS rows x 128 columns of one image (a column strip streamed top to
// bottom), 4 work items (vertically adjacent) per workgroup; a lane holds two cells (a, b) of each row.
//  - Rows of x, l and D pass through a window of three (the row in hand, the one below it for the S faces, the one in flight):
//    the 16-byte loads of row r + 2 are issued before the arithmetic of row r.  Rows are clamped into the image, never tested,
//    and every lane loads (a lane beyond the arrays reads the row's first cells): the count of loads in flight is the same on
//    every path.
//  - A face is evaluated ONCE: per row a lane computes the face a|b, the E face of b and the two S faces.  The W term of a
//    is the other half of the left lane's E face (wave_shr:1); the N terms are the other halves of the S faces of the row
//    above, carried down the strip.  A work item that starts inside an image evaluates the faces above its first row once.
//  - The strip's outer neighbours: per tile, lanes 0...7 load the cell west of the strip for one row each (and the strip's
//    own first cell) and evaluate that face, or the left wall's term; lanes 8...15 load the cell east of it.  A row takes
//    them from there with v_readlane: lane 0's W term and lane 63's E neighbour enter as the `old` operand of the lane
//    shifts, no per-row selects.  The next tile's outer cells are loaded a tile ahead.
//  - Only the last strip (EDGE) knows the right wall, the cells beyond it and the pad column, by per-lane selects.
// Addresses are 64-bit (image base + row base are wave-uniform, the lane adds its column).  No LDS, no waiting.
// partial[img * per_img + tx * cpi + chunk] = the work item's sum of D * g (cpi = work items per strip and image).
__global__ __launch_bounds__(256) void k_vjp(const double *__restrict__ x, const double *__restrict__ lam,
                                             const double *__restrict__ D, int nx, int nxt, int ny, int nimg, int ntx, int cpi,
                                             int kt, double wx, double wy, double ww, double CL, double CR,
                                             double *__restrict__ g, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t gy = (size_t)nimg * (size_t)cpi;
    const size_t wt = (size_t)blockIdx.x * 4u + (size_t)wave;
    if (wt >= (size_t)ntx * gy) return;
    const int tx = (int)(wt / gy);
    const size_t ty = wt % gy;
    const int img = (int)(ty / (size_t)cpi), chunk = (int)(ty - (size_t)img * (size_t)cpi);
    const int l_begin = chunk * VJP_ROWS * kt;                   // rows [l_begin, l_end) of the image
    const int l_end = min(l_begin + VJP_ROWS * kt, ny);
    const int col0 = tx * VJP_COLS, col = col0 + 2 * lane;
    const size_t ibase = (size_t)img * (size_t)ny * (size_t)nx;
    const double *xi = x + ibase, *li = lam + ibase, *Di = D + ibase;
    double *gi = g + ibase;

    auto run = [&](auto edge_tag) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        const bool va = !EDGE || col < nxt, vb = !EDGE || col + 1 < nxt;        // cells of the mesh
        const bool a_last = EDGE && col == nxt - 1, b_last = EDGE && col + 1 == nxt - 1;
        const bool st = !EDGE || col < nx;                                       // lanes inside the arrays
        const int colx = st ? col : 0;
        auto load_row = [&](int r, double2 &xr, double2 &lr, double2 &Dr) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(max(r, 0), ny - 1) * (size_t)nx;       // wave-uniform clamp
            xr = *reinterpret_cast<const double2 *>(xi + rb + colx);
            lr = *reinterpret_cast<const double2 *>(li + rb + colx);
            Dr = *reinterpret_cast<const double2 *>(Di + rb + colx);
        };
        // outer cells of a tile: lane h < 8 row l + h west of the strip, lane 8 + h row l + h east of it; lanes above 15 repeat lane 15
        const int hl = min(lane, 15), hq = hl & 7;
        const bool wwall = tx == 0;
        const int hcol = hl < 8 ? (wwall ? 0 : col0 - 1) : (col0 + VJP_COLS < nxt ? col0 + VJP_COLS : 0);
        struct Outer { double hx, hl, hD, ax, al, aD; };
        auto load_outer = [&](int l, Outer &o) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(l + hq, ny - 1) * (size_t)nx;
            o.hx = xi[rb + hcol]; o.hl = li[rb + hcol]; o.hD = Di[rb + hcol];
            o.ax = xi[rb + col0]; o.al = li[rb + col0]; o.aD = Di[rb + col0];
        };

        double2 xc, lc, Dc, xn, ln, Dn, xf, lf, Df;
        Outer o, o2;
        load_row(l_begin - 1, xf, lf, Df);
        load_row(l_begin, xc, lc, Dc);
        load_row(l_begin + 1, xn, ln, Dn);
        load_outer(l_begin, o);
        // the N terms of the item's first row: the faces above it (nothing above an image's first row)
        double nA, nB, unused;
        vjp_face(Df.x, Dc.x, xf.x, xc.x, lf.x, lc.x, wy, unused, nA);
        vjp_face(Df.y, Dc.y, xf.y, xc.y, lf.y, lc.y, wy, unused, nB);
        if (l_begin == 0) { nA = 0.0; nB = 0.0; }
        double acc = 0.0;
#pragma unroll 1
        for (int l = l_begin; l < l_end; l += VJP_ROWS) {
            load_outer(l + VJP_ROWS, o2);
            double hw;                                           // lanes 0...7: the W term of the strip's first cell in row l + lane
            if (wwall) { const double e = o.ax - CL; hw = ww * (e * o.al); }
            else vjp_face(o.aD, o.hD, o.ax, o.hx, o.al, o.hl, wx, hw, unused);
#pragma unroll
            for (int q = 0; q < VJP_ROWS; ++q) {
                const int r = l + q;
                if (r >= l_end) break;                           // wave-uniform: the item's (or the image's) last rows
                load_row(r + 2, xf, lf, Df);
                const double hwq = vjp_readlane(hw, q);
                const double xEh = vjp_readlane(o.hx, 8 + q), lEh = vjp_readlane(o.hl, 8 + q), DEh = vjp_readlane(o.hD, 8 + q);
                const double xe = dpp_f64_keep<0x130>(xc.x, xEh);    // wave_shl:1, lane 63 keeps the cell east of the strip
                const double le = dpp_f64_keep<0x130>(lc.x, lEh);
                const double De = dpp_f64_keep<0x130>(Dc.x, DEh);
                double mA, mB, eB, eQ, sA, sB, nA2, nB2;
                vjp_face(Dc.x, Dc.y, xc.x, xc.y, lc.x, lc.y, wx, mA, mB);    // a | b
                vjp_face(Dc.y, De, xc.y, xe, lc.y, le, wx, eB, eQ);          // b | the next lane's a
                if constexpr (EDGE) {                                // the right wall
                    const double ea = xc.x - CR, eb = xc.y - CR;
                    if (a_last) mA = ww * (ea * lc.x);
                    if (b_last) eB = ww * (eb * lc.y);
                }
                const double wA = dpp_f64_keep<0x138>(eQ, hwq);      // wave_shr:1, lane 0 keeps the strip's outer W term
                vjp_face(Dc.x, Dn.x, xc.x, xn.x, lc.x, ln.x, wy, sA, nA2);
                vjp_face(Dc.y, Dn.y, xc.y, xn.y, lc.y, ln.y, wy, sB, nB2);
                if (r == ny - 1) { sA = 0.0; sB = 0.0; }             // wave-uniform
                double ga = -(((wA + mA) + nA) + sA);
                double gb = -(((mB + eB) + nB) + sB);
                if (!va || Dc.x == 0) ga = 0.0;
                if (!vb || Dc.y == 0) gb = 0.0;
                if (va) acc += Dc.x * ga;
                if (vb) acc += Dc.y * gb;
                if (st) *reinterpret_cast<double2 *>(gi + (size_t)r * (size_t)nx + col) = make_double2(ga, gb);
                nA = nA2; nB = nB2;
                xc = xn; lc = ln; Dc = Dn; xn = xf; ln = lf; Dn = Df;
            }
            o = o2;
        }
        const double s = wave_sum_to_lane63(acc);
        if (lane == 63) partial[(size_t)img * ((size_t)ntx * cpi) + (size_t)tx * cpi + chunk] = s;
    };
    if (tx == ntx - 1) run(VjpTag<true>{});
    else run(VjpTag<false>{});
}

// One workgroup of 16 waves per image: thread t adds the work items' sums t, t + 1024, ... of its image in that order, the wave
// tree combines the 64 thread sums of a wave, thread 0 adds the 16 wave sums in wave order.  out[img] = sum.
__global__ __launch_bounds__(1024) void k_vjp_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    __shared__ double ws[16];
    const double *p = partial + (size_t)blockIdx.x * per_img;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < per_img; i += 1024) acc += p[i];
    const double s = wave_sum_to_lane63(acc);
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = ws[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) t += ws[w];
        out[blockIdx.x] = t;
    }
}

}  // namespace deff
