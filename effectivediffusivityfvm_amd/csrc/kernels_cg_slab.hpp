// kernels_cg_slab.hpp -- the streaming CG kernels of kernels_cg.hpp for ONE ROW SLAB of an image that is spread over several
// slabs (api_slab.hip, DESIGN.md section 9 "Row slabs"), FP64, gfx950 wave64.  Same table (7 planes in LDS), same row walks
// (cg_dir_rows, cg_update_rows, cg_resid_rows of kernels_cg.hpp, on the slab's window), same scalar steps (cg_alpha_step,
// cg_beta_step, cg_check_step) and admissibility rule (cg_cell_bad), same work items -- 128 columns x kr rows per wave,
// 4 waves per workgroup --, but:
//
//   * kr and the strips come from the WHOLE image (row pitch, NY); a slab cuts its OWNED array rows [own_lo, own_lo + own_h)
//     into items of kr rows from its first owned row.  Array rows outside the mesh [m_lo, m_hi) read as 0, as "outside the
//     image" does in kernels_cg.hpp.
//   * one halo row above and below the owned rows takes part: r there comes from the neighbour (one row per neighbour per
//     iteration, moved by the host loop), p there is kept by this slab itself -- p' = r / A0 + beta p is pointwise, r, beta
//     and the coefficients of a shared row are the same doubles in both slabs, so the item that owns the first (last) owned
//     row also writes p' on the halo row above (below) it and gets the owner's bits.  Halo rows never enter a partial sum.
//   * the scalars are not per image but per slab, and every slab holds the same ones bit for bit: a slab reduces its
//     partials with the fixed order of cg_image_sum to one double per quantity (k_slcg_sum), the slabs' sums are gathered by
//     the host loop, and every slab adds them in slab order ((S0 + S1) + S2) + ... (slcg_total).  Alpha, beta and the done
//     flag follow from these totals alone, so all slabs take the same decision without asking anyone.  No kernel here waits
//     for memory another slab writes: ordering between slabs is stream order and events only.
//
// One slab that is the whole image has no halo row inside the mesh and a total of one sum: its items, their order and every
// sum are those of kernels_cg.hpp on a plain context -- the same bits.  With more slabs the dot products are grouped by
// slab: the field agrees with the one-context CG to rounding, not bit for bit (the status the on-chip form has).
#pragma once
#include "kernels_cg.hpp"

namespace deff {

constexpr int SLCG_SLOT = 3;                   // doubles a slab contributes to a gather (r.r, r.z, b.b; fewer are used elsewhere)

struct CgSlabGeom {
    int nx, ntx, kr;                          // row pitch, strips, rows per item (of the whole image)
    int own_lo, own_h;                        // owned array rows
    int m_lo, m_hi;                           // array rows inside the mesh: [m_lo, m_hi)
    unsigned items;                           // ntx * ceil(own_h / kr): work items (= partial sums) of this slab
};

struct CgSlabItem {
    int col, l0, l1;
    unsigned idx;
};

__device__ __forceinline__ bool slcg_item(const CgSlabGeom &g, int wave, int lane, CgSlabItem &it)
{
    const unsigned wt = blockIdx.x * 4u + (unsigned)wave;
    if (wt >= g.items) return false;
    const int ty = (int)(wt / (unsigned)g.ntx), tx = (int)(wt - (unsigned)ty * g.ntx);
    it.col = tx * CG_COLS + 2 * lane;
    it.l0 = g.own_lo + ty * g.kr;
    it.l1 = min(it.l0 + g.kr, g.own_lo + g.own_h);
    it.idx = wt;
    return true;
}

// The slabs' sums of one quantity (slot `o` of each slab's SLCG_SLOT doubles in `all`), added in slab order; this slab's
// own sum is `mine` (recomputed from its partials: the same bits it published).
__device__ __forceinline__ double slcg_total(const double *__restrict__ all, int nslabs, int me, int o, double mine)
{
    double t = me == 0 ? mine : all[o];
    for (int q = 1; q < nslabs; ++q) t = t + (q == me ? mine : all[(size_t)q * SLCG_SLOT + o]);
    return t;
}

// a slab's window: its array starts at row 0, the rows inside the mesh count
__device__ __forceinline__ CgWin slcg_win(const CgSlabGeom &g) { return CgWin{0, g.m_lo, g.m_hi}; }

// Launch A of a slab.  p_out = z + beta p_in on the owned rows of the item and on the adjacent halo row of the slab's first /
// last item (this slab keeps its p there itself); partial[idx] = p_out . A p_out of the item's owned cells.  cg_dir_rows.
__global__ __launch_bounds__(256) void k_slcg_dir(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                 const double *__restrict__ r, const double *__restrict__ p_in,
                                                 double *__restrict__ p_out, const CgScal *__restrict__ sc, CgSlabGeom g,
                                                 double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgSlabItem it;
    if (!slcg_item(g, wave, lane, it)) return;
    if (sc->done) return;                                        // frozen: no writes
    const bool above = it.l0 == g.own_lo && it.l0 - 1 >= g.m_lo, below = it.l1 == g.own_lo + g.own_h && it.l1 < g.m_hi;
    const double s = cg_dir_rows(tab, code, r, p_in, p_out, slcg_win(g), g.nx, it.col, it.l0, it.l1,
                                 cg_halo_col(g.nx, it.col, lane), sc->restart != 0, sc->beta, above, below);
    if (lane == 63) partial[it.idx] = s;
}

// Launch B of a slab.  x += alpha p, r -= alpha A p on the owned rows (p on the two halo rows as k_slcg_dir left it);
// partial_rz[idx] = r.z, partial_rr[idx] = r.r of the updated r.  cg_update_rows.
__global__ __launch_bounds__(256) void k_slcg_update(const double *__restrict__ tab_g, int nrows,
                                                    const uint16_t *__restrict__ code, const double *__restrict__ p,
                                                    double *__restrict__ x, double *__restrict__ r,
                                                    const CgScal *__restrict__ sc, CgSlabGeom g, double *__restrict__ partial_rz,
                                                    double *__restrict__ partial_rr)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgSlabItem it;
    if (!slcg_item(g, wave, lane, it)) return;
    if (sc->done) return;
    double s1, s2;
    cg_update_rows(tab, code, p, x, r, slcg_win(g), g.nx, it.col, it.l0, it.l1, cg_halo_col(g.nx, it.col, lane), sc->alpha, s1,
                   s2);
    if (lane == 63) { partial_rz[it.idx] = s1; partial_rr[it.idx] = s2; }
}

// r = b - A x on the owned rows (x read as 0 on decoupled cells, and written so; one valid halo row of x above and below);
// partials r.r, r.z, b.b at 3 * idx + 0, 1, 2.  cg_resid_rows.
__global__ __launch_bounds__(256) void k_slcg_resid(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                   double *__restrict__ x, double *__restrict__ r, CgSlabGeom g,
                                                   double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgSlabItem it;
    if (!slcg_item(g, wave, lane, it)) return;
    double s1, s2, s3;
    cg_resid_rows(tab, code, x, r, slcg_win(g), g.nx, it.col, it.l0, it.l1, cg_halo_col(g.nx, it.col, lane), s1, s2, s3);
    if (lane == 63) cg_store3(partial, it.idx, s1, s2, s3);
}

// This slab's sums of `nq` quantities (quantity k: `items` partials at pk[i * st + k * ok]) in the order of cg_image_sum,
// published in its slot for the gather.  One workgroup.  (Not launched for a slab that is the whole image.)
__global__ __launch_bounds__(CG_FIN) void k_slcg_sum(const double *__restrict__ part, unsigned items, int st, size_t ok, int nq,
                                                    double *__restrict__ slot)
{
    __shared__ double ws[4];
    for (int k = 0; k < nq; ++k) {
        const double s = cg_image_sum(part + (size_t)k * ok, items, st, 0, ws);
        if (threadIdx.x == 0) slot[k] = s;
    }
}

// after k_slcg_dir and the gather: alpha = rho / p.Ap (k_cg_alpha on the total)
__global__ __launch_bounds__(CG_FIN) void k_slcg_alpha(const double *__restrict__ part, unsigned items,
                                                      const double *__restrict__ all, int nslabs, int me, CgScal *__restrict__ sc)
{
    __shared__ double ws[4];
    CgScal &s = *sc;
    if (s.done) return;
    const double mine = cg_image_sum(part, items, 1, 0, ws);
    if (threadIdx.x == 0) cg_alpha_step(s, slcg_total(all, nslabs, me, 0, mine));
}

// after k_slcg_update and the gather: one more iteration; stop, or the next beta (k_cg_beta on the totals)
__global__ __launch_bounds__(CG_FIN) void k_slcg_beta(const double *__restrict__ part_rz, const double *__restrict__ part_rr,
                                                     unsigned items, const double *__restrict__ all, int nslabs, int me,
                                                     CgScal *__restrict__ sc, double tol2, long long max_iter)
{
    __shared__ double ws[4];
    CgScal &s = *sc;
    if (s.done) return;
    const double rz1 = cg_image_sum(part_rz, items, 1, 0, ws);
    const double rr1 = cg_image_sum(part_rr, items, 1, 0, ws);
    if (threadIdx.x == 0)
        cg_beta_step(s, slcg_total(all, nslabs, me, 0, rz1), slcg_total(all, nslabs, me, 1, rr1), tol2, max_iter);
}

// after k_slcg_resid and the gather (k_cg_check on the totals).  mode 0: start;  mode 1: the true residual of the finished
// solve -- it stands, or (allow_restart, iterations left) r is the true one now and p restarts from z.  *restarted: 1 then.
__global__ __launch_bounds__(CG_FIN) void k_slcg_check(const double *__restrict__ part, unsigned items,
                                                      const double *__restrict__ all, int nslabs, int me, CgScal *__restrict__ sc,
                                                      double tol2, long long max_iter, int mode, int allow_restart,
                                                      unsigned *restarted)
{
    __shared__ double ws[4];
    CgScal &s = *sc;
    const double rr1 = cg_image_sum(part, items, 3, 0, ws);
    const double rz1 = cg_image_sum(part, items, 3, 1, ws);
    const double bb1 = cg_image_sum(part, items, 3, 2, ws);
    if (threadIdx.x != 0) return;
    const double rr = slcg_total(all, nslabs, me, 0, rr1), rz = slcg_total(all, nslabs, me, 1, rz1),
                 bb = slcg_total(all, nslabs, me, 2, bb1);
    if (cg_check_step(s, rr, rz, bb, tol2, max_iter, mode, allow_restart != 0)) atomicAdd(restarted, 1u);
}

// Admissibility over a slab's window (its array rows inside the mesh): every link between two active cells of the window
// equals its partner bit for bit, and an active row's link out of the mesh (beyond a wall, above mesh row 0, below the last)
// is 0.  A link across the window's edge inside the mesh belongs to the neighbouring slab's window.  The verdict goes into
// the slab's gather slot as a double (0 = admissible), after `pre`: a refusal the host found before the launch.
__global__ __launch_bounds__(256) void k_slcg_admissible(const double *__restrict__ tab_g, int nrows,
                                                        const uint16_t *__restrict__ code, int nx, int m_lo, int m_hi,
                                                        int mesh_top, int mesh_bot, unsigned *flag)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const size_t n = (size_t)nx * (m_hi - m_lo);
    bool bad = false;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        const size_t p = (size_t)m_lo * nx + k;
        if (cg_v<CG_INV>(tab, code[p]) == 0.0) continue;
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx);
        bad |= cg_cell_bad(tab, code, p, j, nx, row > m_lo ? CG_NEIGHBOUR : mesh_top ? CG_WALL : CG_OTHERS,
                           row + 1 < m_hi ? CG_NEIGHBOUR : mesh_bot ? CG_WALL : CG_OTHERS);
    }
    if (bad) atomicOr(flag, 1u);
}

__global__ void k_slcg_verdict(const unsigned *__restrict__ flag, double pre, double *__restrict__ slot)
{
    slot[0] = pre != 0.0 ? pre : (*flag ? 1.0 : 0.0);
    slot[1] = 0.0;
    slot[2] = 0.0;
}

}  // namespace deff
