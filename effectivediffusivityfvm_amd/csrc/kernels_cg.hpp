// kernels_cg.hpp -- Jacobi-preconditioned conjugate gradients on the matrix-free system (16-bit code per cell + a row table of
// its own in LDS), FP64, gfx950 wave64.  Not the reference's algorithm (it has no CG): an opt-in solver that converges to the
// same discrete fixed point A x = b as the weighted Jacobi loop (api_cg.hip).
//
// Table: CG_PLANES planes (A0, 1/A0, aW, aE, aS, aN, b) of LUT_PLANE_STRIDE doubles, built on the host from c->lut_rows; a
// cell's code is the byte offset of its row inside a plane, exactly as in the sweep kernels' table (lut_layout.hpp).  A
// DECOUPLED row (all four links == 0 and b == 0: cells outside the mesh, the pad column, ImpSolid / FloodFill rows, a phase
// that cannot diffuse) is all zeros here, 1/A0 included: its x, p, r and z are 0 and stay 0, so an active row's link into it
// multiplies zeros and the iteration runs on the active block.  "Active" = 1/A0 != 0.
//
// One iteration = two streaming launches + two one-workgroup-per-image reductions:
//   k_cg_dir     p' = z + beta p (z = r / A0, recomputed from r), double-buffered (the neighbours' p' are recomputed from
//                their r and old p), and per-wave partials of p'.Ap' (Ap' only in registers)          26 B/cell
//   k_cg_alpha   alpha = rho / (p'.Ap') per image
//   k_cg_update  Ap' recomputed from p'; x += alpha p', r -= alpha Ap'; partials of r.z and r.r       42 B/cell
//   k_cg_beta    rho' = r.z, ||r||^2; the image's done flag when ||r|| <= rtol ||b||, else beta = rho' / rho
// A finished image is frozen on the device: every kernel returns at once for it (no writes), whatever the host enqueues.
// k_cg_resid (r = b - A x, also zeroes x on decoupled cells) + k_cg_check start the loop and recompute the true residual at
// its end.
//
// Shared bodies: what a step computes is written once, here, and called by every table-form kernel -- these, the folded
// k_cgf_dir / k_cgf_update (kernels_cg_fold.hpp), the listed-slot k_cgs_* (kernels_cg_stream.hpp) and the row-slab k_slcg_*
// (kernels_cg_slab.hpp): the row walks cg_dir_rows, cg_update_rows, cg_resid_rows on a row window (CgWin), the sum of an
// image's partials cg_image_sum, the scalar steps cg_alpha_step, cg_beta_step, cg_check_step, and the admissibility rule
// cg_cell_bad.  A kernel keeps its prologue (table, item, done test), its way of storing partials and its tail.
//
// Determinism: a wave's cells are added by a fixed DPP tree (wave_sum_to_lane63), the partials of an image in index order by
// its own workgroup; work items are numbered image by image with a geometry that depends on (nx, ny) only -- an image of a
// stack gives the bits of a one-image context.  Rows of another image and columns beyond the walls read as 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lut_layout.hpp"
#include "wave_reduce.hpp"

namespace deff {

constexpr int CG_PLANES = 7;
constexpr int CG_A0 = 0, CG_INV = 1, CG_W = 2, CG_E = 3, CG_S = 4, CG_N = 5, CG_B = 6;
constexpr int CG_DOUBLES = CG_PLANES * LUT_PLANE_STRIDE;        // 3640 doubles = 28.4 KiB of LDS
constexpr int CG_COLS = 128;                                    // columns of a work item: 2 per lane
constexpr int CG_FIN = 256;                                     // threads of a reduction workgroup

// per image, on the device
struct CgScal {
    double rho, alpha, beta, bb, rr, rel;
    long long iters;
    int done;                   // 0 running, 1 ||r|| <= rtol ||b|| (recurrence), 2 max_iter, 3 breakdown (p.Ap <= 0)
    int restart;                // next k_cg_dir takes p = z
};

// work items: strips of 128 columns x kr rows; per image ntx * cpi of them, row-major; 4 per workgroup (one per wave)
struct CgGeom {
    int nx, ny, nimg, ntx, cpi, kr;
    unsigned per_img;           // items (= partial sums) per image
};

__device__ __forceinline__ void cg_load_tab(double *tab, const double *__restrict__ g, int nrows)
{
    for (int k = threadIdx.x; k < CG_PLANES * nrows; k += 256) {
        const int pl = k / nrows, r = k - pl * nrows;
        tab[pl * LUT_PLANE_STRIDE + r] = g[pl * LUT_PLANE_STRIDE + r];
    }
    __syncthreads();
}

template <int PLANE>
__device__ __forceinline__ double cg_v(const double *tab, unsigned off)
{
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(tab) + off + PLANE * LUT_PLANE_STRIDE * 8);
}

struct CgItem {
    int img, col, l0, l1;
    size_t base;                // first cell of the image
    unsigned idx;               // partial slot = img * per_img + item
};

__device__ __forceinline__ bool cg_item(const CgGeom &g, int wave, int lane, CgItem &it)
{
    const unsigned wt = blockIdx.x * 4u + (unsigned)wave;
    if (wt >= g.per_img * (unsigned)g.nimg) return false;
    it.img = (int)(wt / g.per_img);
    const unsigned rem = wt - (unsigned)it.img * g.per_img;
    const int ty = (int)(rem / (unsigned)g.ntx), tx = (int)(rem - (unsigned)ty * g.ntx);
    it.col = tx * CG_COLS + 2 * lane;
    it.l0 = ty * g.kr;
    it.l1 = min(it.l0 + g.kr, g.ny);
    it.base = (size_t)it.img * g.ny * g.nx;
    it.idx = wt;
    return true;
}

// A y of a lane's two cells of row l: c = y of the row, n / s = rows above / below, h = the outer neighbour lane 0 (west) or
// lane 63 (east) holds, the others come from the neighbouring lanes
__device__ __forceinline__ double2 cg_apply(const double *tab, unsigned o0, unsigned o1, double2 c, double2 n, double2 s,
                                            double h)
{
    const double w = dpp_f64_keep<0x138>(c.y, h);               // wave_shr:1, lane 0 keeps its outer neighbour
    const double e = dpp_f64_keep<0x130>(c.x, h);               // wave_shl:1, lane 63 keeps its outer neighbour
    double2 a;
    a.x = cg_v<CG_A0>(tab, o0) * c.x + cg_v<CG_W>(tab, o0) * w + cg_v<CG_E>(tab, o0) * c.y + cg_v<CG_S>(tab, o0) * s.x +
          cg_v<CG_N>(tab, o0) * n.x;
    a.y = cg_v<CG_A0>(tab, o1) * c.y + cg_v<CG_W>(tab, o1) * c.x + cg_v<CG_E>(tab, o1) * e + cg_v<CG_S>(tab, o1) * s.y +
          cg_v<CG_N>(tab, o1) * n.y;
    return a;
}

// the outer neighbour of lanes 0 / 63: cell col - 1 / col + 2 if it lies inside the walls, else none
__device__ __forceinline__ int cg_halo_col(int nx, int col, int lane)
{
    const int j = lane == 0 ? col - 1 : col + 2;
    return ((lane == 0 || lane == 63) && j >= 0 && j < nx) ? j : -1;
}

// The rows a walk may read: `base` = offset of the cell (array row 0, column 0), array rows [lo, hi) count, every other row
// reads as 0.  An image of a stack: {img * ny * nx, 0, ny}; a row slab: {0, m_lo, m_hi}.
struct CgWin {
    size_t base;
    int lo, hi;
};
__device__ __forceinline__ CgWin cg_win(const CgGeom &g, const CgItem &it) { return CgWin{it.base, 0, g.ny}; }

// ---- the row walks: ONE body per step, called by every table-form kernel (plain, folded, listed slots, row slab).  A wave
// walks the rows [l0, l1) of its item, two cells per lane from column `col` (row pitch nx, jh = cg_halo_col); the image's
// scalars come in as values.  The wave's sums are returned, valid in lane 63; storing them is the caller's business.

// p_out = z + beta p_in (p_out = z on a restart) on the item's cells; returns p_out . A p_out.  above / below (uniform in the
// wave; a row slab's first / last item alone sets them): also store p' on row l0 - 1 / on row l1.
__device__ __forceinline__ double cg_dir_rows(const double *tab, const uint16_t *__restrict__ code, const double *__restrict__ r,
                                              const double *__restrict__ p_in, double *__restrict__ p_out, const CgWin &w, int nx,
                                              int col, int l0, int l1, int jh, bool restart, double beta, bool above, bool below)
{
    const bool v = col < nx;
    auto pn1 = [&](size_t q) -> double {
        const double z = r[q] * cg_v<CG_INV>(tab, code[q]);
        return restart ? z : z + beta * p_in[q];
    };
    auto pn2 = [&](int l) -> double2 {                           // p' of the lane's two cells of row l (0 outside the window)
        double2 o = make_double2(0.0, 0.0);
        if (v && l >= w.lo && l < w.hi) {
            const size_t q = w.base + (size_t)l * nx + col;
            const unsigned cw = *reinterpret_cast<const unsigned *>(code + q);
            const double2 rr = *reinterpret_cast<const double2 *>(r + q);
            const double2 z = make_double2(rr.x * cg_v<CG_INV>(tab, cw & 0xFFFFu), rr.y * cg_v<CG_INV>(tab, cw >> 16));
            if (restart) o = z;
            else {
                const double2 pp = *reinterpret_cast<const double2 *>(p_in + q);
                o = make_double2(z.x + beta * pp.x, z.y + beta * pp.y);
            }
        }
        return o;
    };
    double2 up = pn2(l0 - 1), cur = pn2(l0);
    if (v && above) *reinterpret_cast<double2 *>(p_out + w.base + (size_t)(l0 - 1) * nx + col) = up;
    double acc = 0.0;
#pragma unroll 1
    for (int l = l0; l < l1; ++l) {
        const double2 dn = pn2(l + 1);
        const size_t q = w.base + (size_t)l * nx + col;
        const double h = jh >= 0 ? pn1(w.base + (size_t)l * nx + jh) : 0.0;
        const unsigned cw = v ? *reinterpret_cast<const unsigned *>(code + q) : 0u;
        const double2 ap = cg_apply(tab, cw & 0xFFFFu, cw >> 16, cur, up, dn, h);
        acc += cur.x * ap.x + cur.y * ap.y;
        if (v) *reinterpret_cast<double2 *>(p_out + q) = cur;
        up = cur;
        cur = dn;
    }
    if (v && below) *reinterpret_cast<double2 *>(p_out + w.base + (size_t)l1 * nx + col) = cur;      // cur = p' of row l1 now
    return wave_sum_to_lane63(acc);
}

// x += alpha p, r -= alpha A p on the item's cells; s_rz = r.z, s_rr = r.r of the updated r.
__device__ __forceinline__ void cg_update_rows(const double *tab, const uint16_t *__restrict__ code, const double *__restrict__ p,
                                               double *__restrict__ x, double *__restrict__ r, const CgWin &w, int nx, int col,
                                               int l0, int l1, int jh, double alpha, double &s_rz, double &s_rr)
{
    const bool v = col < nx;
    auto p2 = [&](int l) -> double2 {
        return (v && l >= w.lo && l < w.hi) ? *reinterpret_cast<const double2 *>(p + w.base + (size_t)l * nx + col)
                                            : make_double2(0.0, 0.0);
    };
    double2 up = p2(l0 - 1), cur = p2(l0);
    double rz = 0.0, rr = 0.0;
#pragma unroll 1
    for (int l = l0; l < l1; ++l) {
        const double2 dn = p2(l + 1);
        const size_t q = w.base + (size_t)l * nx + col;
        const double h = jh >= 0 ? p[w.base + (size_t)l * nx + jh] : 0.0;
        const unsigned cw = v ? *reinterpret_cast<const unsigned *>(code + q) : 0u;
        const unsigned o0 = cw & 0xFFFFu, o1 = cw >> 16;
        const double2 ap = cg_apply(tab, o0, o1, cur, up, dn, h);
        if (v) {
            double2 xx = *reinterpret_cast<const double2 *>(x + q), rv = *reinterpret_cast<const double2 *>(r + q);
            xx.x = xx.x + alpha * cur.x;
            xx.y = xx.y + alpha * cur.y;
            rv.x = rv.x - alpha * ap.x;
            rv.y = rv.y - alpha * ap.y;
            *reinterpret_cast<double2 *>(x + q) = xx;
            *reinterpret_cast<double2 *>(r + q) = rv;
            rz += rv.x * (rv.x * cg_v<CG_INV>(tab, o0)) + rv.y * (rv.y * cg_v<CG_INV>(tab, o1));
            rr += rv.x * rv.x + rv.y * rv.y;
        }
        up = cur;
        cur = dn;
    }
    s_rz = wave_sum_to_lane63(rz);
    s_rr = wave_sum_to_lane63(rr);
}

// r = b - A x on the item's cells (x read as 0 on decoupled cells, and written so); s_rr = r.r, s_rz = r.z, s_bb = b.b.
__device__ __forceinline__ void cg_resid_rows(const double *tab, const uint16_t *__restrict__ code, double *__restrict__ x,
                                              double *__restrict__ r, const CgWin &w, int nx, int col, int l0, int l1, int jh,
                                              double &s_rr, double &s_rz, double &s_bb)
{
    const bool v = col < nx;
    auto x1 = [&](size_t q) -> double { return cg_v<CG_INV>(tab, code[q]) != 0.0 ? x[q] : 0.0; };
    auto x2 = [&](int l) -> double2 {
        double2 o = make_double2(0.0, 0.0);
        if (v && l >= w.lo && l < w.hi) {
            const size_t q = w.base + (size_t)l * nx + col;
            const unsigned cw = *reinterpret_cast<const unsigned *>(code + q);
            const double2 xx = *reinterpret_cast<const double2 *>(x + q);
            o.x = cg_v<CG_INV>(tab, cw & 0xFFFFu) != 0.0 ? xx.x : 0.0;
            o.y = cg_v<CG_INV>(tab, cw >> 16) != 0.0 ? xx.y : 0.0;
        }
        return o;
    };
    double2 up = x2(l0 - 1), cur = x2(l0);
    double rr = 0.0, rz = 0.0, bb = 0.0;
#pragma unroll 1
    for (int l = l0; l < l1; ++l) {
        const double2 dn = x2(l + 1);
        const size_t q = w.base + (size_t)l * nx + col;
        const double h = jh >= 0 ? x1(w.base + (size_t)l * nx + jh) : 0.0;
        const unsigned cw = v ? *reinterpret_cast<const unsigned *>(code + q) : 0u;
        const unsigned o0 = cw & 0xFFFFu, o1 = cw >> 16;
        const double2 ax = cg_apply(tab, o0, o1, cur, up, dn, h);
        if (v) {
            const double b0 = cg_v<CG_B>(tab, o0), b1 = cg_v<CG_B>(tab, o1);
            const double2 rv = make_double2(b0 - ax.x, b1 - ax.y);
            *reinterpret_cast<double2 *>(r + q) = rv;
            *reinterpret_cast<double2 *>(x + q) = cur;
            rr += rv.x * rv.x + rv.y * rv.y;
            rz += rv.x * (rv.x * cg_v<CG_INV>(tab, o0)) + rv.y * (rv.y * cg_v<CG_INV>(tab, o1));
            bb += b0 * b0 + b1 * b1;
        }
        up = cur;
        cur = dn;
    }
    s_rr = wave_sum_to_lane63(rr), s_rz = wave_sum_to_lane63(rz), s_bb = wave_sum_to_lane63(bb);
}

// the partials r.r, r.z, b.b of item idx, as k_cg_check and its kin read them: at 3 * idx + 0, 1, 2
__device__ __forceinline__ void cg_store3(double *__restrict__ partial, unsigned idx, double s1, double s2, double s3)
{
    partial[3 * (size_t)idx] = s1;
    partial[3 * (size_t)idx + 1] = s2;
    partial[3 * (size_t)idx + 2] = s3;
}

// Launch A.  p_out = z + beta p_in on every cell of the item, partial[idx] = p_out . A p_out of the item's cells.
__global__ __launch_bounds__(256) void k_cg_dir(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                const double *__restrict__ r, const double *__restrict__ p_in,
                                                double *__restrict__ p_out, const CgScal *__restrict__ sc, CgGeom g,
                                                double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    if (sc[it.img].done) return;                                 // frozen image: no writes
    const double s = cg_dir_rows(tab, code, r, p_in, p_out, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                                 cg_halo_col(g.nx, it.col, lane), sc[it.img].restart != 0, sc[it.img].beta, false, false);
    if (lane == 63) partial[it.idx] = s;
}

// Launch B.  x += alpha p, r -= alpha A p; partial_rz[idx] = r.z, partial_rr[idx] = r.r of the updated r.
__global__ __launch_bounds__(256) void k_cg_update(const double *__restrict__ tab_g, int nrows,
                                                   const uint16_t *__restrict__ code, const double *__restrict__ p,
                                                   double *__restrict__ x, double *__restrict__ r,
                                                   const CgScal *__restrict__ sc, CgGeom g, double *__restrict__ partial_rz,
                                                   double *__restrict__ partial_rr)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    if (sc[it.img].done) return;
    double s1, s2;
    cg_update_rows(tab, code, p, x, r, cg_win(g, it), g.nx, it.col, it.l0, it.l1, cg_halo_col(g.nx, it.col, lane),
                   sc[it.img].alpha, s1, s2);
    if (lane == 63) { partial_rz[it.idx] = s1; partial_rr[it.idx] = s2; }
}

// r = b - A x of every image (x read as 0 on decoupled cells, and written so); partials r.r, r.z, b.b at 3 * idx + 0, 1, 2.
__global__ __launch_bounds__(256) void k_cg_resid(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                  double *__restrict__ x, double *__restrict__ r, CgGeom g,
                                                  double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    double s1, s2, s3;
    cg_resid_rows(tab, code, x, r, cg_win(g, it), g.nx, it.col, it.l0, it.l1, cg_halo_col(g.nx, it.col, lane), s1, s2,
                  s3);
    if (lane == 63) cg_store3(partial, it.idx, s1, s2, s3);
}

// Sum of one image's per_img partials (pp = its first one; stride `st`, offset `o`) in a fixed order: thread t adds t,
// t + 256, ... in index order, the wave tree, then thread 0 the four wave sums in wave order.  Valid in thread 0.
__device__ __forceinline__ double cg_image_sum(const double *pp, unsigned per_img, int st, int o, double *ws)
{
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < per_img; i += CG_FIN) acc += pp[(size_t)i * st + o];
    const double s = wave_sum_to_lane63(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// ---- the scalar steps of an image (or of a row slab: the same rule on the slabs' totals), run by one thread

// after the direction launch: alpha = rho / p.Ap, or breakdown
__device__ __forceinline__ void cg_alpha_step(CgScal &s, double pap)
{
    if (pap > 0.0 && pap <= 1.7976931348623157e308) s.alpha = s.rho / pap;
    else { s.alpha = 0.0; s.done = 3; }
    s.restart = 0;
}

// after the update launch: one more iteration of the image; stop, or the next beta
__device__ __forceinline__ void cg_beta_step(CgScal &s, double rz, double rr, double tol2, long long max_iter)
{
    s.iters += 1;
    s.rr = rr;
    if (rr <= tol2 * s.bb) s.done = 1;
    else if (s.iters >= max_iter) s.done = 2;
    else {
        s.beta = rz / s.rho;
        s.rho = rz;
    }
}

// after the true residual r = b - A x.  mode 0: start (||b||^2, rho, iteration 0);  mode 1: the true residual of a finished
// image -- it stands as the result, or (allow, iterations left) the recurrence drifted: r is the true one now, restart p
// from z.  Returns whether the image restarted (mode 1 only).
__device__ __forceinline__ bool cg_check_step(CgScal &s, double rr, double rz, double bb, double tol2, long long max_iter,
                                              int mode, bool allow)
{
    s.rr = rr;
    s.rel = bb > 0.0 ? __builtin_sqrt(rr) / __builtin_sqrt(bb) : (rr == 0.0 ? 0.0 : __builtin_inf());
    const bool ok = rr <= tol2 * bb;
    if (mode == 0) {
        s.bb = bb;
        s.iters = 0;
        s.rho = rz;
        s.alpha = 0.0;
        s.beta = 0.0;
        s.restart = 1;
        s.done = ok ? 1 : (max_iter <= 0 ? 2 : 0);
        return false;
    }
    if (ok || !allow || s.iters >= max_iter) return false;
    s.rho = rz;
    s.beta = 0.0;
    s.restart = 1;
    s.done = 0;
    return true;
}

// after k_cg_dir: alpha = rho / p.Ap
__global__ __launch_bounds__(CG_FIN) void k_cg_alpha(const double *__restrict__ part, unsigned per_img, CgScal *__restrict__ sc)
{
    __shared__ double ws[4];
    CgScal &s = sc[blockIdx.x];
    if (s.done) return;
    const double pap = cg_image_sum(part + (size_t)blockIdx.x * per_img, per_img, 1, 0, ws);
    if (threadIdx.x == 0) cg_alpha_step(s, pap);
}

// after k_cg_update: one more iteration of the image; stop, or the next beta
__global__ __launch_bounds__(CG_FIN) void k_cg_beta(const double *__restrict__ part_rz, const double *__restrict__ part_rr,
                                                    unsigned per_img, CgScal *__restrict__ sc, double tol2, long long max_iter)
{
    __shared__ double ws[4];
    CgScal &s = sc[blockIdx.x];
    if (s.done) return;
    const double rz = cg_image_sum(part_rz + (size_t)blockIdx.x * per_img, per_img, 1, 0, ws);
    const double rr = cg_image_sum(part_rr + (size_t)blockIdx.x * per_img, per_img, 1, 0, ws);
    if (threadIdx.x == 0) cg_beta_step(s, rz, rr, tol2, max_iter);
}

// after k_cg_resid: cg_check_step of every image.  *restarted (mode 1) counts the images that go on.
__global__ __launch_bounds__(CG_FIN) void k_cg_check(const double *__restrict__ part, unsigned per_img, CgScal *__restrict__ sc,
                                                     double tol2, long long max_iter, int mode, int allow_restart,
                                                     unsigned *restarted)
{
    __shared__ double ws[4];
    const double *pp = part + (size_t)blockIdx.x * per_img * 3;
    const double rr = cg_image_sum(pp, per_img, 3, 0, ws);
    const double rz = cg_image_sum(pp, per_img, 3, 1, ws);
    const double bb = cg_image_sum(pp, per_img, 3, 2, ws);
    if (threadIdx.x != 0) return;
    if (cg_check_step(sc[blockIdx.x], rr, rz, bb, tol2, max_iter, mode, allow_restart != 0)) atomicAdd(restarted, 1u);
}

// The admissibility rule for one cell: whether the ACTIVE cell p (column j of its row; cd = the codes p indexes) has a bad
// link -- one to an active neighbour that differs from its partner bit for bit, or a non-zero one out of the image (beyond a
// wall).  What lies above and below the cell's row:
enum CgEdge {
    CG_NEIGHBOUR,               // a row of the same window: the link is compared with its partner
    CG_WALL,                    // nothing (first / last row of the mesh): the link must be 0
    CG_OTHERS,                  // a row inside the mesh that belongs to another slab's window: not checked here
};
__device__ __forceinline__ bool cg_cell_bad(const double *tab, const uint16_t *__restrict__ cd, size_t p, int j, int nx,
                                            CgEdge above, CgEdge below)
{
    auto same = [](double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); };
    const unsigned me = cd[p];
    bool bad = false;
    if (j > 0) {
        const unsigned o = cd[p - 1];
        if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_W>(tab, me), cg_v<CG_E>(tab, o));
    } else bad |= cg_v<CG_W>(tab, me) != 0.0;
    if (j + 1 < nx) {
        const unsigned o = cd[p + 1];
        if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_E>(tab, me), cg_v<CG_W>(tab, o));
    } else bad |= cg_v<CG_E>(tab, me) != 0.0;
    if (above == CG_NEIGHBOUR) {
        const unsigned o = cd[p - nx];
        if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_N>(tab, me), cg_v<CG_S>(tab, o));
    } else if (above == CG_WALL) bad |= cg_v<CG_N>(tab, me) != 0.0;
    if (below == CG_NEIGHBOUR) {
        const unsigned o = cd[p + nx];
        if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_S>(tab, me), cg_v<CG_N>(tab, o));
    } else if (below == CG_WALL) bad |= cg_v<CG_S>(tab, me) != 0.0;
    return bad;
}

// Admissibility of (table, codes) for CG: every link between two active cells equals its partner bit for bit, and an active
// row's link to a cell outside its image (beyond a wall, the first / last row) is 0.  Raises *flag on a mismatch.
__global__ __launch_bounds__(256) void k_cg_admissible(const double *__restrict__ tab_g, int nrows,
                                                       const uint16_t *__restrict__ code, int nx, int rows, int ny,
                                                       unsigned *flag)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const size_t n = (size_t)nx * rows;
    bool bad = false;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        if (cg_v<CG_INV>(tab, code[p]) == 0.0) continue;
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx), li = row % ny;
        bad |= cg_cell_bad(tab, code, p, j, nx, li > 0 ? CG_NEIGHBOUR : CG_WALL, li + 1 < ny ? CG_NEIGHBOUR : CG_WALL);
    }
    if (bad) atomicOr(flag, 1u);
}

}  // namespace deff
