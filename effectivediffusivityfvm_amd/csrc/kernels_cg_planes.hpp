// kernels_cg_planes.hpp -- the conjugate-gradient iteration of kernels_cg.hpp on the explicit coefficient planes
// (a0, aW, aE, aS, aN, b, one double per cell each) instead of the 16-bit row code and the row table: for systems that have
// no row dictionary (a diffusivity that varies cell by cell, a caller's own assembly, more distinct rows than a dictionary
// holds, dictionaries disabled).  Tuning key "cg_planes" (api_cg.hip, DESIGN.md section 9 "Planes").  FP64, gfx950 wave64.
//
// Only where a row comes from differs from the table form.  The work items (cg_item), the partial-sum slots, the expressions
// and their order (cgp_apply = cg_apply with the row's values passed in), the wave tree and the per-image reductions
// (k_cg_alpha, k_cg_beta, k_cg_check) are the table form's, so a system that has a dictionary gives the same bits either way.
//
//   k_cgp_prepare  one pass over the planes: the plane cg_inv (0 on a DECOUPLED cell -- four zero links and b == 0, the table
//                  form's rule --, else 1 / a0: an IEEE division, the double the host's cg_table computes) and the
//                  admissibility of the system, which the table form checks on the host (cg_table) and in k_cg_admissible
//   k_cgp_dir      p' = r inv + beta p, A p' from the five planes, stored as q; partials of p'.q                80 B/cell
//   k_cgp_update   x += alpha p', r -= alpha q; partials of r.(r inv) and r.r: a stream without neighbours     56 B/cell
//   k_cgp_resid    r = b - A x (x read as 0 and written as 0 on decoupled cells); partials r.r, r.z, b.b
//
// A decoupled row counts as all zeros, as in the table: its a0 is replaced by 0 where it is multiplied (its links and b are
// zeros already), so an identity row (the pad column, ImpSolid rows: a0 = 1) contributes what the table's row 0 contributes.
// The coefficient planes are read once per iteration and loaded non-temporally: the caches are left to r, p and inv, which
// neighbouring items and the next launch read again.  There is no table in LDS: registers alone bound the occupancy.
// k_cgp_dir and k_cgp_update issue the loads of row l + 1 before the arithmetic of row l needs row l's.
// Their row walks are cgp_dir_rows and cgp_update_rows below, which the folded k_cgpf_dir / k_cgpf_update call too.
#pragma once
#include <type_traits>
#include "kernels_cg.hpp"

namespace deff {

constexpr unsigned CGP_FLAG_SYM = 1u;           // a link differs from its partner, or an active row links out of its image
constexpr unsigned CGP_FLAG_ROW = 2u;           // an active row is not admissible (a0, 1 / a0, links, b)

struct CgpPlanes {
    const double *a0, *aW, *aE, *aS, *aN, *b;
};

typedef double cgp_v2d __attribute__((ext_vector_type(2)));
typedef const char __attribute__((address_space(1))) *cgp_gptr;      // a byte address in global memory

// two cells of a coefficient plane, streamed past the caches
__device__ __forceinline__ double2 cgp_ldc2(const double *p)
{
    const cgp_v2d v = __builtin_nontemporal_load(reinterpret_cast<const cgp_v2d *>(p));
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ double2 cgp_ld2(const double *p) { return *reinterpret_cast<const double2 *>(p); }
__device__ __forceinline__ void cgp_st2(double *p, double2 v) { *reinterpret_cast<double2 *>(p) = v; }

// a wave-uniform address as a scalar base (global address space: an integer would come back as a generic pointer)
__device__ __forceinline__ cgp_gptr cgp_uniform(const double *a)
{
    const unsigned long long u = (unsigned long long)a;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return (cgp_gptr)(((unsigned long long)hi << 32) | lo);
}
// scalar base + the lane's 32-bit byte offset
__device__ __forceinline__ double2 cgp_gld2(cgp_gptr row, unsigned off)
{
    const cgp_v2d t = *(const cgp_v2d __attribute__((address_space(1))) *)(row + off);
    return make_double2(t.x, t.y);
}
__device__ __forceinline__ double2 cgp_gldc2(cgp_gptr row, unsigned off)
{
    const cgp_v2d t = __builtin_nontemporal_load((const cgp_v2d __attribute__((address_space(1))) *)(row + off));
    return make_double2(t.x, t.y);
}
__device__ __forceinline__ double cgp_gld1(cgp_gptr row, unsigned off) { return *(const double __attribute__((address_space(1))) *)(row + off); }
__device__ __forceinline__ void cgp_gst2(cgp_gptr row, unsigned off, double2 t)
{
    cgp_v2d w;
    w.x = t.x;
    w.y = t.y;
    *(cgp_v2d __attribute__((address_space(1))) *)(row + off) = w;
}

// the matrix rows of a lane's two cells
struct CgpRow {
    double2 a0, aW, aE, aS, aN;
};

__device__ __forceinline__ CgpRow cgp_row(const CgpPlanes &A, size_t q, bool v)
{
    CgpRow o;
    o.a0 = o.aW = o.aE = o.aS = o.aN = make_double2(0.0, 0.0);
    if (v) {
        o.a0 = cgp_ldc2(A.a0 + q);
        o.aW = cgp_ldc2(A.aW + q);
        o.aE = cgp_ldc2(A.aE + q);
        o.aS = cgp_ldc2(A.aS + q);
        o.aN = cgp_ldc2(A.aN + q);
    }
    return o;
}

// cg_apply with the rows' values instead of table offsets; act: bit 0 / 1 = the lane's first / second cell is active
__device__ __forceinline__ double2 cgp_apply(const CgpRow &m, unsigned act, double2 c, double2 n, double2 s, double h)
{
    const double w = dpp_f64_keep<0x138>(c.y, h);               // wave_shr:1, lane 0 keeps its outer neighbour
    const double e = dpp_f64_keep<0x130>(c.x, h);               // wave_shl:1, lane 63 keeps its outer neighbour
    const double d0 = (act & 1u) ? m.a0.x : 0.0, d1 = (act & 2u) ? m.a0.y : 0.0;
    double2 a;
    a.x = d0 * c.x + m.aW.x * w + m.aE.x * c.y + m.aS.x * s.x + m.aN.x * n.x;
    a.y = d1 * c.y + m.aW.y * c.x + m.aE.y * e + m.aS.y * s.y + m.aN.y * n.y;
    return a;
}

__device__ __forceinline__ unsigned cgp_act(double2 inv) { return (inv.x != 0.0 ? 1u : 0u) | (inv.y != 0.0 ? 2u : 0u); }

__device__ __forceinline__ bool cgp_decoupled(const CgpPlanes &A, size_t p)
{
    return A.aW[p] == 0.0 && A.aE[p] == 0.0 && A.aS[p] == 0.0 && A.aN[p] == 0.0 && A.b[p] == 0.0;
}

// inv = 0 on decoupled cells, 1 / a0 elsewhere; *flag |= CGP_FLAG_ROW for an active row that is not admissible (cg_table's
// conditions), CGP_FLAG_SYM for what k_cg_admissible refuses
__global__ __launch_bounds__(256) void k_cgp_prepare(CgpPlanes A, int nx, int rows, int ny, double *__restrict__ inv,
                                                     unsigned *flag)
{
    const size_t n = (size_t)nx * rows;
    unsigned bad = 0;
    auto same = [](double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); };
    auto finite = [](double a) { return __builtin_fabs(a) <= 1.7976931348623157e308; };        // false for NaN
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const double a0 = A.a0[p], aW = A.aW[p], aE = A.aE[p], aS = A.aS[p], aN = A.aN[p], b = A.b[p];
        if (aW == 0.0 && aE == 0.0 && aS == 0.0 && aN == 0.0 && b == 0.0) {
            inv[p] = 0.0;
            continue;
        }
        const double iv = 1.0 / a0;
        inv[p] = iv;
        const bool normal = __builtin_fabs(iv) >= 2.2250738585072014e-308 && finite(iv);
        if (!(a0 > 0.0) || !normal || !finite(a0) || !finite(aW) || !finite(aE) || !finite(aS) || !finite(aN) || !finite(b))
            bad |= CGP_FLAG_ROW;
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx), li = row % ny;
        if (j > 0) {
            if (!cgp_decoupled(A, p - 1) && !same(aW, A.aE[p - 1])) bad |= CGP_FLAG_SYM;
        } else if (aW != 0.0) bad |= CGP_FLAG_SYM;
        if (j + 1 < nx) {
            if (!cgp_decoupled(A, p + 1) && !same(aE, A.aW[p + 1])) bad |= CGP_FLAG_SYM;
        } else if (aE != 0.0) bad |= CGP_FLAG_SYM;
        if (li > 0) {
            if (!cgp_decoupled(A, p - nx) && !same(aN, A.aS[p - nx])) bad |= CGP_FLAG_SYM;
        } else if (aN != 0.0) bad |= CGP_FLAG_SYM;
        if (li + 1 < ny) {
            if (!cgp_decoupled(A, p + nx) && !same(aS, A.aN[p + nx])) bad |= CGP_FLAG_SYM;
        } else if (aS != 0.0) bad |= CGP_FLAG_SYM;
    }
    if (bad) atomicOr(flag, bad);
}

// A right-hand side that is not the system's own b (deff_solve_adjoint): w[p] = 0 on the cells k_cgp_prepare found decoupled
// (inv == 0; a select, so a NaN there goes too), so that r = w - A x is 0 there as it is for b.  In place.
__global__ __launch_bounds__(256) void k_cgp_mask_rhs(const double *__restrict__ inv, size_t n, double *__restrict__ w)
{
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256)
        if (inv[p] == 0.0) w[p] = 0.0;
}

// what p' of a lane's two cells is made of (zeros outside the image)
struct CgpRaw2 {
    double2 r, inv, p;
};
struct CgpRaw1 {
    double r, inv, p;
};

// ---- the row walks of the iteration: one body per step, shared by k_cgp_* and the folded k_cgpf_* (kernels_cg_fold.hpp).
// As in kernels_cg.hpp: rows [l0, l1) of the item, two cells per lane from column `col`, the window `w`, the image's scalars
// as values; the wave's sums are returned, valid in lane 63, and the caller stores them.

// p_out = r inv + beta p_in and q = A p_out on every cell of the item; returns p_out . q.
// Rolling window: in front of row l's arithmetic the loads of row l + 1 are issued -- its matrix rows, its halo cell and what
// p' of row l + 2 is made of --, so a row's arithmetic never waits for what its own turn asked for.  90 VGPRs in k_cgp_dir:
// five waves per SIMD, the table form's occupancy (how the loads are written below is what keeps it there).
__device__ __forceinline__ double cgp_dir_rows(const CgpPlanes &A, const double *__restrict__ inv, const double *__restrict__ r,
                                               const double *__restrict__ p_in, double *__restrict__ p_out,
                                               double *__restrict__ q_out, const CgWin &w, int nx, int col, int l0, int l1, int jh,
                                               bool restart, double beta)
{
    const bool v = col < nx;
    // Loads without branches: a load that a branch may skip makes the count of loads in flight unknown where the next wait is
    // placed, and the wait becomes one for all of them.  So every lane loads from a clamped address (a lane beyond the row's
    // end reads the row's first cells, a row outside the image the nearest one inside) and what may not count is zeroed
    // afterwards (pn2, pn1, the lanes' A p').
    // Addresses: the row's first cell (uniform in the wave: a scalar base, kept apart from the lane's part by readfirstlane)
    // + the lane's byte offset in the row (32 bits, one register for every array); a 64-bit address per array and lane would
    // cost the fifth wave per SIMD.
    const unsigned cb = v ? (unsigned)col * 8u : 0u, hb = (unsigned)max(jh, 0) * 8u;
    auto row_of = [&](const double *a, int l) { return cgp_uniform(a + w.base + (size_t)min(max(l, w.lo), w.hi - 1) * nx); };
    auto inside = [&](int l) { return v && l >= w.lo && l < w.hi; };
    auto raw2 = [&](int l) -> CgpRaw2 {
        CgpRaw2 o;
        o.r = cgp_gld2(row_of(r, l), cb);
        o.inv = cgp_gld2(row_of(inv, l), cb);
        o.p = cgp_gld2(row_of(p_in, l), cb);
        return o;
    };
    auto pn2 = [&](const CgpRaw2 &o, int l) -> double2 {           // p' of the lane's two cells of row l (0 outside)
        const double2 z = make_double2(o.r.x * o.inv.x, o.r.y * o.inv.y);
        const double2 t = restart ? z : make_double2(z.x + beta * o.p.x, z.y + beta * o.p.y);
        return inside(l) ? t : make_double2(0.0, 0.0);
    };
    auto raw1 = [&](int l) -> CgpRaw1 {
        CgpRaw1 o;
        o.r = cgp_gld1(row_of(r, l), hb);
        o.inv = cgp_gld1(row_of(inv, l), hb);
        o.p = cgp_gld1(row_of(p_in, l), hb);
        return o;
    };
    auto pn1 = [&](const CgpRaw1 &o) -> double {
        const double z = o.r * o.inv;
        const double t = restart ? z : z + beta * o.p;
        return jh >= 0 ? t : 0.0;
    };
    auto mrow = [&](int l) -> CgpRow {
        CgpRow o;
        o.a0 = cgp_gldc2(row_of(A.a0, l), cb);
        o.aW = cgp_gldc2(row_of(A.aW, l), cb);
        o.aE = cgp_gldc2(row_of(A.aE, l), cb);
        o.aS = cgp_gldc2(row_of(A.aS, l), cb);
        o.aN = cgp_gldc2(row_of(A.aN, l), cb);
        return o;
    };
    const CgpRaw2 r0 = raw2(l0 - 1), r1 = raw2(l0);
    CgpRow ma = mrow(l0), mb = ma;
    CgpRaw2 rd = raw2(l0 + 1);                                  // row l + 1
    CgpRaw1 hd = raw1(l0);
    double2 up = pn2(r0, l0 - 1), cur = pn2(r1, l0);
    unsigned act = cgp_act(r1.inv);
    double acc = 0.0;
    // Row l: its matrix is in `m`, the next row's goes into `mn` -- the two sets take turns, because a copy from one register
    // to another would wait for the load it copies, and with it for everything the turn has just asked for.  MORE: row l + 1
    // belongs to the item; the item's last row asks for nothing.
    auto step = [&](auto more_c, int l, const CgpRow &m, CgpRow &mn) {
        constexpr bool MORE = decltype(more_c)::value;
        // the next row's matrix first; then what the previous turn asked for is used up (it was issued behind this row's
        // matrix, so that has arrived too), and its registers take the requests of the turn after
        if constexpr (MORE) mn = mrow(l + 1);
        const double2 dn = pn2(rd, l + 1);
        const double h = pn1(hd);
        const unsigned act_dn = cgp_act(rd.inv);
        if constexpr (MORE) {
            __builtin_amdgcn_sched_barrier(0);
            rd = raw2(l + 2);
            hd = raw1(l + 1);
        }
        double2 ap = cgp_apply(m, act, cur, up, dn, h);
        if (!v) ap = make_double2(0.0, 0.0);
        acc += cur.x * ap.x + cur.y * ap.y;
        if (v) {
            cgp_gst2(row_of(p_out, l), cb, cur);
            cgp_gst2(row_of(q_out, l), cb, ap);
        }
        up = cur;
        cur = dn;
        act = act_dn;
    };
    const std::true_type more;
    const std::false_type last;
    int l = l0;
#pragma unroll 1
    for (; l + 2 < l1; l += 2) {
        step(more, l, ma, mb);
        step(more, l + 1, mb, ma);
    }
    if (l + 1 < l1) {
        step(more, l, ma, mb);
        step(last, l + 1, mb, ma);
    } else step(last, l, ma, mb);
    return wave_sum_to_lane63(acc);
}

struct CgpUpd {
    double2 p, q, x, r, inv;
};

// x += alpha p, r -= alpha q on the item's cells; s_rz = r.(r inv), s_rr = r.r of the updated r.  (x and r are read and
// written through the same pointers: no __restrict__.)
__device__ __forceinline__ void cgp_update_rows(const double *__restrict__ inv, const double *__restrict__ p,
                                                const double *__restrict__ qv, double *x, double *r, const CgWin &w, int nx,
                                                int col, int l0, int l1, double alpha, double &s_rz, double &s_rr)
{
    const bool v = col < nx;
    // as in cgp_dir_rows: loads without branches from a scalar row base, two register sets that take turns
    const unsigned cb = v ? (unsigned)col * 8u : 0u;
    auto row_of = [&](const double *a, int l) { return cgp_uniform(a + w.base + (size_t)l * nx); };
    auto load = [&](int l) -> CgpUpd {
        CgpUpd o;
        o.p = cgp_gld2(row_of(p, l), cb);
        o.q = cgp_gld2(row_of(qv, l), cb);
        o.x = cgp_gld2(row_of(x, l), cb);
        o.r = cgp_gld2(row_of(r, l), cb);
        o.inv = cgp_gld2(row_of(inv, l), cb);
        return o;
    };
    double rz = 0.0, rr = 0.0;
    auto step = [&](int l, const CgpUpd &d) {
        if (v) {
            double2 xx = d.x, rv = d.r;
            xx.x = xx.x + alpha * d.p.x;
            xx.y = xx.y + alpha * d.p.y;
            rv.x = rv.x - alpha * d.q.x;
            rv.y = rv.y - alpha * d.q.y;
            cgp_gst2(row_of(x, l), cb, xx);
            cgp_gst2(row_of(r, l), cb, rv);
            rz += rv.x * (rv.x * d.inv.x) + rv.y * (rv.y * d.inv.y);
            rr += rv.x * rv.x + rv.y * rv.y;
        }
    };
    CgpUpd da = load(l0), db = da;
    int l = l0;
#pragma unroll 1
    for (; l + 2 < l1; l += 2) {
        db = load(l + 1);
        step(l, da);
        da = load(l + 2);
        step(l + 1, db);
    }
    if (l + 1 < l1) {
        db = load(l + 1);
        step(l, da);
        step(l + 1, db);
    } else step(l, da);
    s_rz = wave_sum_to_lane63(rz);
    s_rr = wave_sum_to_lane63(rr);
}

// Launch A.  p_out = r inv + beta p_in and q = A p_out on every cell of the item, partial[idx] = p_out . q.
__global__ __launch_bounds__(256) void k_cgp_dir(CgpPlanes A, const double *__restrict__ inv, const double *__restrict__ r,
                                                 const double *__restrict__ p_in, double *__restrict__ p_out,
                                                 double *__restrict__ q_out, const CgScal *__restrict__ sc, CgGeom g,
                                                 double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    if (sc[it.img].done) return;                                 // frozen image: no writes
    const double s = cgp_dir_rows(A, inv, r, p_in, p_out, q_out, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                                  cg_halo_col(g.nx, it.col, lane), sc[it.img].restart != 0, sc[it.img].beta);
    if (lane == 63) partial[it.idx] = s;
}

// Launch B.  x += alpha p, r -= alpha q; partial_rz[idx] = r.(r inv), partial_rr[idx] = r.r of the updated r.
__global__ __launch_bounds__(256) void k_cgp_update(const double *__restrict__ inv, const double *__restrict__ p,
                                                    const double *__restrict__ qv, double *x, double *r, const CgScal *__restrict__ sc, CgGeom g,
                                                    double *__restrict__ partial_rz, double *__restrict__ partial_rr)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    if (sc[it.img].done) return;
    double s1, s2;
    cgp_update_rows(inv, p, qv, x, r, cg_win(g, it), g.nx, it.col, it.l0, it.l1, sc[it.img].alpha, s1, s2);
    if (lane == 63) { partial_rz[it.idx] = s1; partial_rr[it.idx] = s2; }
}

// r = b - A x of every image (x read as 0 on decoupled cells, and written so); partials r.r, r.z, b.b at 3 * idx + 0, 1, 2.
__global__ __launch_bounds__(256) void k_cgp_resid(CgpPlanes A, const double *__restrict__ inv, double *__restrict__ x,
                                                   double *__restrict__ r, CgGeom g, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    const bool v = it.col < g.nx;
    const int jh = cg_halo_col(g.nx, it.col, lane);
    auto x1 = [&](size_t q) -> double { return inv[q] != 0.0 ? x[q] : 0.0; };
    auto x2 = [&](int l, double2 &iv) -> double2 {
        double2 o = make_double2(0.0, 0.0);
        iv = make_double2(0.0, 0.0);
        if (v && l >= 0 && l < g.ny) {
            const size_t q = it.base + (size_t)l * g.nx + it.col;
            iv = cgp_ld2(inv + q);
            const double2 xx = cgp_ld2(x + q);
            o.x = iv.x != 0.0 ? xx.x : 0.0;
            o.y = iv.y != 0.0 ? xx.y : 0.0;
        }
        return o;
    };
    double2 iup, icur, idn;
    double2 up = x2(it.l0 - 1, iup), cur = x2(it.l0, icur);
    double rr = 0.0, rz = 0.0, bb = 0.0;
#pragma unroll 1
    for (int l = it.l0; l < it.l1; ++l) {
        const double2 dn = x2(l + 1, idn);
        const size_t q = it.base + (size_t)l * g.nx + it.col;
        const double h = jh >= 0 ? x1(it.base + (size_t)l * g.nx + jh) : 0.0;
        const CgpRow m = cgp_row(A, q, v);
        const double2 ax = cgp_apply(m, cgp_act(icur), cur, up, dn, h);
        if (v) {
            const double2 bv = cgp_ldc2(A.b + q);
            const double2 rv = make_double2(bv.x - ax.x, bv.y - ax.y);
            cgp_st2(r + q, rv);
            cgp_st2(x + q, cur);
            rr += rv.x * rv.x + rv.y * rv.y;
            rz += rv.x * (rv.x * icur.x) + rv.y * (rv.y * icur.y);
            bb += bv.x * bv.x + bv.y * bv.y;
        }
        up = cur;
        cur = dn;
        icur = idn;
    }
    const double s1 = wave_sum_to_lane63(rr), s2 = wave_sum_to_lane63(rz), s3 = wave_sum_to_lane63(bb);
    if (lane == 63) cg_store3(partial, it.idx, s1, s2, s3);
}

}  // namespace deff
