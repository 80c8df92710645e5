// kernels_sens.hpp -- the Deff gradient: g[p] = dDeff_raw / dD[p] of a converged field, one streaming pass over x and D
// (gfx950, wave64, FP64; nothing like it in the reference).
//
// The system is self-adjoint: Deff_raw = 2E / (CR - CL)^2 with E = 1/2 sum over faces of g_f (dx_f)^2 (the two wall
// half-faces included), and at the solution dDeff_raw / dg_f = (dx_f)^2 / (CR - CL)^2.  The chain rule through the harmonic
// mean H = 2 Dp Dq / (Dp + Dq) is local: dH / dDp = 2 (Dq / (Dp + Dq))^2.  Per cell p, one term per face (weights as the
// assembly's, fvm_row.hpp: W / E faces carry wx = dy / dx, N / S faces wy = dx / dy, a wall ww = dy / (dx / 2)):
//   interior face to q   s = Dp + Dq;  t = (s == 0) ? 0 : Dq / s;  e = xp - xq;  c = (2.0 * (t * t)) * (w * (e * e))
//   left / right wall    e = xp - CL (CR);  c = ww * (e * e)
//   no face (an image's first and last row)   c = +0.0
//   g[p] = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL)),  and g[p] = 0 where D[p] == 0 (the field there is CG's 0, not a
//   limit).  The pad column of an odd mesh width gets 0.
// s, e * e and w are the same bits seen from either cell of a face (IEEE addition and multiplication commute, (-e)(-e) = e e),
// so w * (e * e) is evaluated ONCE per face and gives the term of both cells with one division each (sens_face).
// tests/sensitivity_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
//
// The second output, euler[img] = sum over the image's cells of D[p] * g[p], equals Deff_raw of the exact solution (Deff is
// homogeneous of degree 1 in D: Euler's identity), a check that needs no reference.  ORDER of that sum: a lane adds its
// cells top to bottom through its work item (first cell of its pair, then the second), the 64 lane sums of a wave are
// combined by wave_reduce.hpp's fixed DPP tree (row_shr 1, 2, 3, 4, 8, then row_bcast 15 and 31: lane 63 holds the sum), and
// k_sens_final (one workgroup of 16 waves per image) has thread t add the work items' sums t, t + 1024, ... in that order,
// the same tree per wave, and thread 0 the 16 wave sums in wave order.  The order depends on the launch geometry only: the
// same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_reduce.hpp"

namespace deff {

constexpr int SENS_ROWS = 8;                     // rows per tile
constexpr int SENS_COLS = 128;                   // columns per strip: 2 per lane
template <bool V> struct SensTag { static constexpr bool value = V; };

// One interior face between cells p and q, weight w: cp = the term of p, cq = the term of q.
__device__ __forceinline__ void sens_face(double Dp, double Dq, double xp, double xq, double w, double &cp, double &cq)
{
    const double s = Dp + Dq;
    const double e = xp - xq;
    const double wee = w * (e * e);
    const double tq = (s == 0) ? 0 : Dq / s;
    const double tp = (s == 0) ? 0 : Dp / s;
    cp = (2.0 * (tq * tq)) * wee;
    cq = (2.0 * (tp * tp)) * wee;
}

__device__ __forceinline__ double sens_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One wave per work item = `kt` consecutive tiles of SENS_ROWS rows x 128 columns of one image (a column strip streamed top to
// bottom), 4 work items (vertically adjacent) per workgroup; a lane holds two cells (a, b) of each row.
//  - Rows of x and D pass through a window of three (the row in hand, the one below it for the S faces, the one in flight):
//    the 16-byte loads of row r + 2 are issued before the arithmetic of row r.  Rows are clamped into the image, never tested.
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
__global__ __launch_bounds__(256) void k_sens(const double *__restrict__ x, const double *__restrict__ D, int nx, int nxt, int ny,
                                              int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                              double CR, double den, double *__restrict__ g, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t gy = (size_t)nimg * (size_t)cpi;
    const size_t wt = (size_t)blockIdx.x * 4u + (size_t)wave;
    if (wt >= (size_t)ntx * gy) return;
    const int tx = (int)(wt / gy);
    const size_t ty = wt % gy;
    const int img = (int)(ty / (size_t)cpi), chunk = (int)(ty - (size_t)img * (size_t)cpi);
    const int l_begin = chunk * SENS_ROWS * kt;                  // rows [l_begin, l_end) of the image
    const int l_end = min(l_begin + SENS_ROWS * kt, ny);
    const int col0 = tx * SENS_COLS, col = col0 + 2 * lane;
    const size_t ibase = (size_t)img * (size_t)ny * (size_t)nx;
    const double *xi = x + ibase, *Di = D + ibase;
    double *gi = g + ibase;

    auto run = [&](auto edge_tag) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        const bool va = !EDGE || col < nxt, vb = !EDGE || col + 1 < nxt;        // cells of the mesh
        const bool a_last = EDGE && col == nxt - 1, b_last = EDGE && col + 1 == nxt - 1;
        const bool st = !EDGE || col < nx;                                       // lanes inside the arrays
        const int colx = st ? col : 0;
        auto load_row = [&](int li, double2 &xr, double2 &Dr) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(max(li, 0), ny - 1) * (size_t)nx;      // wave-uniform clamp
            xr = *reinterpret_cast<const double2 *>(xi + rb + colx);
            Dr = *reinterpret_cast<const double2 *>(Di + rb + colx);
        };
        // outer cells of a tile: lane h < 8 row l + h west of the strip, lane 8 + h row l + h east of it; lanes above 15 repeat lane 15
        const int hl = min(lane, 15), hq = hl & 7;
        const bool wwall = tx == 0;
        const int hcol = hl < 8 ? (wwall ? 0 : col0 - 1) : (col0 + SENS_COLS < nxt ? col0 + SENS_COLS : 0);
        auto load_outer = [&](int l, double &hx, double &hD, double &ax, double &aD) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(l + hq, ny - 1) * (size_t)nx;
            hx = xi[rb + hcol]; hD = Di[rb + hcol];
            ax = xi[rb + col0]; aD = Di[rb + col0];
        };

        double2 xc, Dc, xn, Dn, xf, Df;
        double hx, hD, ax, aD, hx2, hD2, ax2, aD2;
        load_row(l_begin - 1, xf, Df);
        load_row(l_begin, xc, Dc);
        load_row(l_begin + 1, xn, Dn);
        load_outer(l_begin, hx, hD, ax, aD);
        // the N terms of the item's first row: the faces above it (nothing above an image's first row)
        double nA, nB, unused;
        sens_face(Df.x, Dc.x, xf.x, xc.x, wy, unused, nA);
        sens_face(Df.y, Dc.y, xf.y, xc.y, wy, unused, nB);
        if (l_begin == 0) { nA = 0.0; nB = 0.0; }
        double acc = 0.0;
#pragma unroll 1
        for (int l = l_begin; l < l_end; l += SENS_ROWS) {
            load_outer(l + SENS_ROWS, hx2, hD2, ax2, aD2);
            double hw;                                           // lanes 0...7: the W term of the strip's first cell in row l + lane
            if (wwall) { const double e = ax - CL; hw = ww * (e * e); }
            else sens_face(aD, hD, ax, hx, wx, hw, unused);
#pragma unroll
            for (int q = 0; q < SENS_ROWS; ++q) {
                const int r = l + q;
                if (r >= l_end) break;                           // wave-uniform: the item's (or the image's) last rows
                load_row(r + 2, xf, Df);
                const double hwq = sens_readlane(hw, q);
                const double xEh = sens_readlane(hx, 8 + q), DEh = sens_readlane(hD, 8 + q);
                const double xe = dpp_f64_keep<0x130>(xc.x, xEh);    // wave_shl:1, lane 63 keeps the cell east of the strip
                const double De = dpp_f64_keep<0x130>(Dc.x, DEh);
                double mA, mB, eB, eQ, sA, sB, nA2, nB2;
                sens_face(Dc.x, Dc.y, xc.x, xc.y, wx, mA, mB);       // a | b
                sens_face(Dc.y, De, xc.y, xe, wx, eB, eQ);           // b | the next lane's a
                if constexpr (EDGE) {                                // the right wall
                    const double ea = xc.x - CR, eb = xc.y - CR;
                    if (a_last) mA = ww * (ea * ea);
                    if (b_last) eB = ww * (eb * eb);
                }
                const double wA = dpp_f64_keep<0x138>(eQ, hwq);      // wave_shr:1, lane 0 keeps the strip's outer W term
                sens_face(Dc.x, Dn.x, xc.x, xn.x, wy, sA, nA2);
                sens_face(Dc.y, Dn.y, xc.y, xn.y, wy, sB, nB2);
                if (r == ny - 1) { sA = 0.0; sB = 0.0; }             // wave-uniform
                double ga = (((wA + mA) + nA) + sA) / den;
                double gb = (((mB + eB) + nB) + sB) / den;
                if (!va || Dc.x == 0) ga = 0.0;
                if (!vb || Dc.y == 0) gb = 0.0;
                if (va) acc += Dc.x * ga;
                if (vb) acc += Dc.y * gb;
                if (st) *reinterpret_cast<double2 *>(gi + (size_t)r * (size_t)nx + col) = make_double2(ga, gb);
                nA = nA2; nB = nB2;
                xc = xn; Dc = Dn; xn = xf; Dn = Df;
            }
            hx = hx2; hD = hD2; ax = ax2; aD = aD2;
        }
        const double s = wave_sum_to_lane63(acc);
        if (lane == 63) partial[(size_t)img * ((size_t)ntx * cpi) + (size_t)tx * cpi + chunk] = s;
    };
    if (tx == ntx - 1) run(SensTag<true>{});
    else run(SensTag<false>{});
}

// One workgroup of 16 waves per image: thread t adds the work items' sums t, t + 1024, ... of its image in that order, the wave
// tree combines the 64 thread sums of a wave, thread 0 adds the 16 wave sums in wave order.  out[img] = sum.
__global__ __launch_bounds__(1024) void k_sens_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
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
