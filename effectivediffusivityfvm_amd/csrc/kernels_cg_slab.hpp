// kernels_cg_slab.hpp -- the streaming CG kernels of kernels_cg.hpp for ONE ROW SLAB of an image that is spread over several
// slabs (api_slab.hip, DESIGN.md section 9 "Row slabs"), FP64, gfx950 wave64.  Same table (7 planes in LDS), same cg_apply,
// same DPP wave sum, same work items -- 128 columns x kr rows per wave, 4 waves per workgroup --, but:
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

__device__ __forceinline__ int slcg_halo_col(const CgSlabGeom &g, const CgSlabItem &it, int lane)
{
    const int j = lane == 0 ? it.col - 1 : it.col + 2;
    return ((lane == 0 || lane == 63) && j >= 0 && j < g.nx) ? j : -1;
}

// The slabs' sums of one quantity (slot `o` of each slab's SLCG_SLOT doubles in `all`), added in slab order; this slab's
// own sum is `mine` (recomputed from its partials: the same bits it published).
__device__ __forceinline__ double slcg_total(const double *__restrict__ all, int nslabs, int me, int o, double mine)
{
    double t = me == 0 ? mine : all[o];
    for (int q = 1; q < nslabs; ++q) t = t + (q == me ? mine : all[(size_t)q * SLCG_SLOT + o]);
    return t;
}

// Launch A of a slab.  p_out = z + beta p_in on the owned rows of the item and on the adjacent halo row of the slab's first /
// last item; partial[idx] = p_out . A p_out of the item's owned cells.
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
    const bool restart = sc->restart != 0;
    const double beta = sc->beta;
    const bool v = it.col < g.nx;
    const int jh = slcg_halo_col(g, it, lane);
    auto pn1 = [&](size_t q) -> double {
        const double z = r[q] * cg_v<CG_INV>(tab, code[q]);
        return restart ? z : z + beta * p_in[q];
    };
    auto pn2 = [&](int l) -> double2 {                           // p' of the lane's two cells of row l (0 outside the mesh)
        double2 o = make_double2(0.0, 0.0);
        if (v && l >= g.m_lo && l < g.m_hi) {
            const size_t q = (size_t)l * g.nx + it.col;
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
    double2 up = pn2(it.l0 - 1), cur = pn2(it.l0);
    // the halo row above the slab's first owned row: this slab keeps its p itself
    if (v && it.l0 == g.own_lo && it.l0 - 1 >= g.m_lo) *reinterpret_cast<double2 *>(p_out + (size_t)(it.l0 - 1) * g.nx + it.col) = up;
    double acc = 0.0;
#pragma unroll 1
    for (int l = it.l0; l < it.l1; ++l) {
        const double2 dn = pn2(l + 1);
        const size_t q = (size_t)l * g.nx + it.col;
        const double h = jh >= 0 ? pn1((size_t)l * g.nx + jh) : 0.0;
        const unsigned cw = v ? *reinterpret_cast<const unsigned *>(code + q) : 0u;
        const double2 ap = cg_apply(tab, cw & 0xFFFFu, cw >> 16, cur, up, dn, h);
        acc += cur.x * ap.x + cur.y * ap.y;
        if (v) *reinterpret_cast<double2 *>(p_out + q) = cur;
        up = cur;
        cur = dn;
    }
    // ... and the halo row below its last owned row (cur = p' of row l1 now)
    if (v && it.l1 == g.own_lo + g.own_h && it.l1 < g.m_hi) *reinterpret_cast<double2 *>(p_out + (size_t)it.l1 * g.nx + it.col) = cur;
    const double s = wave_sum_to_lane63(acc);
    if (lane == 63) partial[it.idx] = s;
}

// Launch B of a slab.  x += alpha p, r -= alpha A p on the owned rows (p on the two halo rows as k_slcg_dir left it);
// partial_rz[idx] = r.z, partial_rr[idx] = r.r of the updated r.
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
    const double alpha = sc->alpha;
    const bool v = it.col < g.nx;
    const int jh = slcg_halo_col(g, it, lane);
    auto p2 = [&](int l) -> double2 {
        return (v && l >= g.m_lo && l < g.m_hi) ? *reinterpret_cast<const double2 *>(p + (size_t)l * g.nx + it.col)
                                                : make_double2(0.0, 0.0);
    };
    double2 up = p2(it.l0 - 1), cur = p2(it.l0);
    double rz = 0.0, rr = 0.0;
#pragma unroll 1
    for (int l = it.l0; l < it.l1; ++l) {
        const double2 dn = p2(l + 1);
        const size_t q = (size_t)l * g.nx + it.col;
        const double h = jh >= 0 ? p[(size_t)l * g.nx + jh] : 0.0;
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
    const double s1 = wave_sum_to_lane63(rz);
    const double s2 = wave_sum_to_lane63(rr);
    if (lane == 63) { partial_rz[it.idx] = s1; partial_rr[it.idx] = s2; }
}

// r = b - A x on the owned rows (x read as 0 on decoupled cells, and written so; one valid halo row of x above and below);
// partials r.r, r.z, b.b at 3 * idx + 0, 1, 2.
__global__ __launch_bounds__(256) void k_slcg_resid(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                   double *__restrict__ x, double *__restrict__ r, CgSlabGeom g,
                                                   double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgSlabItem it;
    if (!slcg_item(g, wave, lane, it)) return;
    const bool v = it.col < g.nx;
    const int jh = slcg_halo_col(g, it, lane);
    auto x1 = [&](size_t q) -> double { return cg_v<CG_INV>(tab, code[q]) != 0.0 ? x[q] : 0.0; };
    auto x2 = [&](int l) -> double2 {
        double2 o = make_double2(0.0, 0.0);
        if (v && l >= g.m_lo && l < g.m_hi) {
            const size_t q = (size_t)l * g.nx + it.col;
            const unsigned cw = *reinterpret_cast<const unsigned *>(code + q);
            const double2 xx = *reinterpret_cast<const double2 *>(x + q);
            o.x = cg_v<CG_INV>(tab, cw & 0xFFFFu) != 0.0 ? xx.x : 0.0;
            o.y = cg_v<CG_INV>(tab, cw >> 16) != 0.0 ? xx.y : 0.0;
        }
        return o;
    };
    double2 up = x2(it.l0 - 1), cur = x2(it.l0);
    double rr = 0.0, rz = 0.0, bb = 0.0;
#pragma unroll 1
    for (int l = it.l0; l < it.l1; ++l) {
        const double2 dn = x2(l + 1);
        const size_t q = (size_t)l * g.nx + it.col;
        const double h = jh >= 0 ? x1((size_t)l * g.nx + jh) : 0.0;
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
    const double s1 = wave_sum_to_lane63(rr), s2 = wave_sum_to_lane63(rz), s3 = wave_sum_to_lane63(bb);
    if (lane == 63) {
        partial[3 * (size_t)it.idx] = s1;
        partial[3 * (size_t)it.idx + 1] = s2;
        partial[3 * (size_t)it.idx + 2] = s3;
    }
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
    if (threadIdx.x == 0) {
        const double pap = slcg_total(all, nslabs, me, 0, mine);
        if (pap > 0.0 && pap <= 1.7976931348623157e308) s.alpha = s.rho / pap;
        else { s.alpha = 0.0; s.done = 3; }
        s.restart = 0;
    }
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
    if (threadIdx.x == 0) {
        const double rz = slcg_total(all, nslabs, me, 0, rz1), rr = slcg_total(all, nslabs, me, 1, rr1);
        s.iters += 1;
        s.rr = rr;
        if (rr <= tol2 * s.bb) s.done = 1;
        else if (s.iters >= max_iter) s.done = 2;
        else {
            s.beta = rz / s.rho;
            s.rho = rz;
        }
    }
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
    } else if (!ok && allow_restart && s.iters < max_iter) {
        s.rho = rz;
        s.beta = 0.0;
        s.restart = 1;
        s.done = 0;
        atomicAdd(restarted, 1u);
    }
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
    auto same = [](double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); };
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        const size_t p = (size_t)m_lo * nx + k;
        const unsigned me = code[p];
        if (cg_v<CG_INV>(tab, me) == 0.0) continue;
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx);
        if (j > 0) {
            const unsigned o = code[p - 1];
            if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_W>(tab, me), cg_v<CG_E>(tab, o));
        } else bad |= cg_v<CG_W>(tab, me) != 0.0;
        if (j + 1 < nx) {
            const unsigned o = code[p + 1];
            if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_E>(tab, me), cg_v<CG_W>(tab, o));
        } else bad |= cg_v<CG_E>(tab, me) != 0.0;
        if (row > m_lo) {
            const unsigned o = code[p - nx];
            if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_N>(tab, me), cg_v<CG_S>(tab, o));
        } else if (mesh_top) bad |= cg_v<CG_N>(tab, me) != 0.0;
        if (row + 1 < m_hi) {
            const unsigned o = code[p + nx];
            if (cg_v<CG_INV>(tab, o) != 0.0) bad |= !same(cg_v<CG_S>(tab, me), cg_v<CG_N>(tab, o));
        } else if (mesh_bot) bad |= cg_v<CG_S>(tab, me) != 0.0;
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
