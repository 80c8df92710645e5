// kernels_cg_volume.hpp -- volumes: the 7-point system of an nx x ny x nz mesh on the unit cube (fvm_row3, fvm_row.hpp) and the
// plane form's conjugate-gradient iteration (kernels_cg_planes.hpp) on it.  FP64, gfx950 wave64.  DESIGN.md section 16.
//
// Layout: a volume is ONE tall image of ny * nz rows, slice k = rows [k * ny, (k + 1) * ny).  The N / S links are zero on the
// first / last row of every slice (the assembly gives that), so the 2-D kernels would already iterate nz uncoupled slices;
// the planes aB and aF couple row l to rows l - ny and l + ny.  Work items (cg_item on nx x ny*nz), partial-sum slots, the wave
// tree and the per-image reductions are the plane form's: items may straddle slice borders, which needs no special case.
//
//   k_assemble_volume_from_D  k_assemble_from_D's shape: the planes a0, aW, aE, aS, aN, aB, aF, b from a D volume
//   k_cgv_prepare             k_cgp_prepare with the two z links: cg_inv and the admissibility of the system
//   k_cgv_dir                 k_cgp_dir with the back and front rows: p' = r inv + beta p, q = A p', partials of p'.q
//   k_cgv_resid               k_cgp_resid with the two z terms: r = b - A x; partials r.r, r.z, b.b
// k_cgp_update, k_cg_alpha, k_cg_beta and k_cg_check serve unchanged (they read no neighbour and no matrix).
//
// With aB = aF = 0 (a volume of one slice) the z terms add + 0.0 to sums that are not - 0.0: the bits are the 2-D plane form's.
#pragma once
#include "fvm_row.hpp"
#include "kernels_cg_planes.hpp"
#include "kernels_setup.hpp"

namespace deff {

// the z links of a volume beside its CgpPlanes; ny = rows of a slice (0: not a volume -- every 2-D caller)
struct CgvLinks {
    const double *aB = nullptr, *aF = nullptr;
    int ny = 0;
};

// General assembly of a volume from a per-cell D array: k_assemble_from_D's shape (clamped neighbour reads, the identity row
// on the pad column).  rows = ny * nz.
__global__ __launch_bounds__(256) void k_assemble_volume_from_D(const double *__restrict__ D, int nx, int nxt, int ny, int nz,
                                                                double dx, double dy, double dz, double CL, double CR, CoefSoA c,
                                                                double *__restrict__ aB, double *__restrict__ aF)
{
    const size_t sp = (size_t)ny * nx, n = sp * nz;              // cells of a slice, of the volume
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx), k = row / ny, li = row - k * ny;
        FvmRow3 r;
        if (j >= nxt) {
            r.a0 = 1; r.aW = 0; r.aE = 0; r.aS = 0; r.aN = 0; r.aB = 0; r.aF = 0; r.b = 0;
        } else {
            // clamped neighbour reads; values at clamped positions are unused
            const double Dp = D[p];
            const double Dw = D[j > 0 ? p - 1 : p];
            const double De = D[j < nxt - 1 ? p + 1 : p];
            const double Ds = D[li < ny - 1 ? p + nx : p];
            const double Dn = D[li > 0 ? p - nx : p];
            const double Db = D[k > 0 ? p - sp : p];
            const double Df = D[k < nz - 1 ? p + sp : p];
            r = fvm_row3(Dp, Dw, De, Ds, Dn, Db, Df, pos_class(j, nxt), pos_class(li, ny), pos_class_z(k, nz), dx, dy, dz, CL, CR);
        }
        c.a0[p] = r.a0; c.aW[p] = r.aW; c.aE[p] = r.aE; c.aS[p] = r.aS; c.aN[p] = r.aN; c.b[p] = r.b;
        aB[p] = r.aB; aF[p] = r.aF;
    }
}

__device__ __forceinline__ bool cgv_decoupled(const CgpPlanes &A, const CgvLinks &Z, size_t p)
{
    return cgp_decoupled(A, p) && Z.aB[p] == 0.0 && Z.aF[p] == 0.0;
}

// k_cgp_prepare on a volume of rows = ny * nz rows (Z.ny = ny): a cell is decoupled when all six links and b are zero; the
// bit-for-bit symmetry test also takes aB[p] against aF[p - ny * nx] and aF[p] against aB[p + ny * nx]; a z link out of the
// volume is a symmetry failure.
__global__ __launch_bounds__(256) void k_cgv_prepare(CgpPlanes A, CgvLinks Z, int nx, int rows, double *__restrict__ inv,
                                                     unsigned *flag)
{
    const int ny = Z.ny;
    const size_t n = (size_t)nx * rows, sp = (size_t)ny * nx;
    unsigned bad = 0;
    auto same = [](double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); };
    auto finite = [](double a) { return __builtin_fabs(a) <= 1.7976931348623157e308; };        // false for NaN
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const double a0 = A.a0[p], aW = A.aW[p], aE = A.aE[p], aS = A.aS[p], aN = A.aN[p], aB = Z.aB[p], aF = Z.aF[p], b = A.b[p];
        if (aW == 0.0 && aE == 0.0 && aS == 0.0 && aN == 0.0 && aB == 0.0 && aF == 0.0 && b == 0.0) {
            inv[p] = 0.0;
            continue;
        }
        const double iv = 1.0 / a0;
        inv[p] = iv;
        const bool normal = __builtin_fabs(iv) >= 2.2250738585072014e-308 && finite(iv);
        if (!(a0 > 0.0) || !normal || !finite(a0) || !finite(aW) || !finite(aE) || !finite(aS) || !finite(aN) || !finite(aB) ||
            !finite(aF) || !finite(b))
            bad |= CGP_FLAG_ROW;
        const int row = (int)(p / nx), j = (int)(p - (size_t)row * nx), li = row % ny;
        if (j > 0) {
            if (!cgv_decoupled(A, Z, p - 1) && !same(aW, A.aE[p - 1])) bad |= CGP_FLAG_SYM;
        } else if (aW != 0.0) bad |= CGP_FLAG_SYM;
        if (j + 1 < nx) {
            if (!cgv_decoupled(A, Z, p + 1) && !same(aE, A.aW[p + 1])) bad |= CGP_FLAG_SYM;
        } else if (aE != 0.0) bad |= CGP_FLAG_SYM;
        if (li > 0) {
            if (!cgv_decoupled(A, Z, p - nx) && !same(aN, A.aS[p - nx])) bad |= CGP_FLAG_SYM;
        } else if (aN != 0.0) bad |= CGP_FLAG_SYM;
        if (li + 1 < ny) {
            if (!cgv_decoupled(A, Z, p + nx) && !same(aS, A.aN[p + nx])) bad |= CGP_FLAG_SYM;
        } else if (aS != 0.0) bad |= CGP_FLAG_SYM;
        if (row >= ny) {
            if (!cgv_decoupled(A, Z, p - sp) && !same(aB, Z.aF[p - sp])) bad |= CGP_FLAG_SYM;
        } else if (aB != 0.0) bad |= CGP_FLAG_SYM;
        if (row + ny < rows) {
            if (!cgv_decoupled(A, Z, p + sp) && !same(aF, Z.aB[p + sp])) bad |= CGP_FLAG_SYM;
        } else if (aF != 0.0) bad |= CGP_FLAG_SYM;
    }
    if (bad) atomicOr(flag, bad);
}

// the z links of a lane's two cells
struct CgvRow {
    double2 aB, aF;
};

// cgp_apply's sum with the back and front terms added behind it, left to right:
// d0 c + aW w + aE e + aS s + aN n + aB bk + aF f
__device__ __forceinline__ double2 cgv_apply(const CgpRow &m, const CgvRow &z, unsigned act, double2 c, double2 n, double2 s,
                                             double h, double2 bk, double2 f)
{
    double2 a = cgp_apply(m, act, c, n, s, h);
    a.x = a.x + z.aB.x * bk.x + z.aF.x * f.x;
    a.y = a.y + z.aB.y * bk.y + z.aF.y * f.y;
    return a;
}

// cgp_dir_rows with the back and front rows: p' of the cells at rows l - ny and l + ny is recomputed from r, inv and p_in
// by the N / S rows' expression (pn2), so its owner stores the same double; rows outside the window read as 0.  The loads of
// the two rows travel with the halo's: those of row l + 1 are issued in front of row l's arithmetic, branch-free from clamped
// addresses, and what may not count is zeroed afterwards.
__device__ __forceinline__ double cgv_dir_rows(const CgpPlanes &A, const CgvLinks &Z, const double *__restrict__ inv,
                                               const double *__restrict__ r, const double *__restrict__ p_in,
                                               double *__restrict__ p_out, double *__restrict__ q_out, const CgWin &w, int nx,
                                               int col, int l0, int l1, int jh, bool restart, double beta)
{
    const bool v = col < nx;
    const int sl = Z.ny;
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
    auto zrow = [&](int l) -> CgvRow {
        CgvRow o;
        o.aB = cgp_gldc2(row_of(Z.aB, l), cb);
        o.aF = cgp_gldc2(row_of(Z.aF, l), cb);
        return o;
    };
    const CgpRaw2 r0 = raw2(l0 - 1), r1 = raw2(l0);
    CgpRow ma = mrow(l0), mb = ma;
    CgvRow za = zrow(l0), zb = za;
    CgpRaw2 rd = raw2(l0 + 1);                                  // row l + 1
    CgpRaw1 hd = raw1(l0);
    CgpRaw2 bd = raw2(l0 - sl), fd = raw2(l0 + sl);             // the back and front rows of row l
    double2 up = pn2(r0, l0 - 1), cur = pn2(r1, l0);
    unsigned act = cgp_act(r1.inv);
    double acc = 0.0;
    // as cgp_dir_rows: two sets of matrix registers take turns; MORE: row l + 1 belongs to the item
    auto step = [&](auto more_c, int l, const CgpRow &m, CgpRow &mn, const CgvRow &z, CgvRow &zn) {
        constexpr bool MORE = decltype(more_c)::value;
        if constexpr (MORE) {
            mn = mrow(l + 1);
            zn = zrow(l + 1);
        }
        const double2 dn = pn2(rd, l + 1);
        const double h = pn1(hd);
        const unsigned act_dn = cgp_act(rd.inv);
        const double2 bk = pn2(bd, l - sl), f = pn2(fd, l + sl);
        if constexpr (MORE) {
            __builtin_amdgcn_sched_barrier(0);
            rd = raw2(l + 2);
            hd = raw1(l + 1);
            bd = raw2(l + 1 - sl);
            fd = raw2(l + 1 + sl);
        }
        double2 ap = cgv_apply(m, z, act, cur, up, dn, h, bk, f);
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
        step(more, l, ma, mb, za, zb);
        step(more, l + 1, mb, ma, zb, za);
    }
    if (l + 1 < l1) {
        step(more, l, ma, mb, za, zb);
        step(last, l + 1, mb, ma, zb, za);
    } else step(last, l, ma, mb, za, zb);
    return wave_sum_to_lane63(acc);
}

// Launch A of a volume.  p_out = r inv + beta p_in and q = A p_out on every cell of the item, partial[idx] = p_out . q.
__global__ __launch_bounds__(256) void k_cgv_dir(CgpPlanes A, CgvLinks Z, const double *__restrict__ inv,
                                                 const double *__restrict__ r, const double *__restrict__ p_in,
                                                 double *__restrict__ p_out, double *__restrict__ q_out,
                                                 const CgScal *__restrict__ sc, CgGeom g, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    if (sc[it.img].done) return;                                 // frozen: no writes
    const double s = cgv_dir_rows(A, Z, inv, r, p_in, p_out, q_out, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                                  cg_halo_col(g.nx, it.col, lane), sc[it.img].restart != 0, sc[it.img].beta);
    if (lane == 63) partial[it.idx] = s;
}

// r = b - A x of the volume (x read as 0 on decoupled cells, and written so); partials r.r, r.z, b.b at 3 * idx + 0, 1, 2.
__global__ __launch_bounds__(256) void k_cgv_resid(CgpPlanes A, CgvLinks Z, const double *__restrict__ inv, double *__restrict__ x,
                                                   double *__restrict__ r, CgGeom g, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    const bool v = it.col < g.nx;
    const int jh = cg_halo_col(g.nx, it.col, lane), sl = Z.ny;
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
    double2 iup, icur, idn, iz;
    double2 up = x2(it.l0 - 1, iup), cur = x2(it.l0, icur);
    double rr = 0.0, rz = 0.0, bb = 0.0;
#pragma unroll 1
    for (int l = it.l0; l < it.l1; ++l) {
        const double2 dn = x2(l + 1, idn);
        const double2 bk = x2(l - sl, iz), f = x2(l + sl, iz);
        const size_t q = it.base + (size_t)l * g.nx + it.col;
        const double h = jh >= 0 ? x1(it.base + (size_t)l * g.nx + jh) : 0.0;
        const CgpRow m = cgp_row(A, q, v);
        CgvRow z;
        z.aB = z.aF = make_double2(0.0, 0.0);
        if (v) {
            z.aB = cgp_ldc2(Z.aB + q);
            z.aF = cgp_ldc2(Z.aF + q);
        }
        const double2 ax = cgv_apply(m, z, cgp_act(icur), cur, up, dn, h, bk, f);
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
