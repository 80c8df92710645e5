// kernels_cg_image_planes.hpp -- k_cg_image's iteration (kernels_cg_image.hpp: a whole small image on ONE compute unit) with
// the matrix rows taken from the explicit coefficient planes instead of the 16-bit codes and the row table: for systems that
// have no row dictionary (kernels_cg_planes.hpp) and for the side solves on the forward matrix (deff_solve_adjoint,
// deff_solve_tangent, deff_solve_adjoint_tangent).  Tuning key "cg_onchip_planes" (api_cg.hip, DESIGN.md section 9 "On chip,
// planes"), deff_get_plan "cg_impl" 4.
//
// The same as in k_cg_image: the workgroup of 1024 threads, the flat pair mapping j = t + 1024 k, p in LDS (128 KiB), r in
// registers, the phases (A) / (B) / (C), the order of every sum, the scalars' write-back, the frozen-image skip and the image
// loop.  What differs: a pair's row is five 16-byte loads (a0, aW, aE, aS, aN) and its 1 / a0 a sixth (cg_inv, which
// k_cgp_prepare writes for every plane-form solve), all from global memory -- 640 KiB of coefficients per 128 x 128 image fit
// neither LDS nor registers beside the vectors, so every iteration reads them again, from L2 or Infinity Cache.  To read them
// ONCE per iteration, q = A p is held in registers from (B) to (C), in the 32 VGPRs that hold x in k_cg_image, and x lives in
// global memory: (C) reads and writes the lane's own cells of it (the field is current after every iteration).  Per cell and
// iteration:
//   (A) inv 8 B | (B) five planes 40 B | (C) inv 8 B, x 8 B read + 8 B written                       = 72 B (64 read, 8 written)
// against 96 B with A p computed again in (C) as k_cg_image does (measured: DESIGN.md).  Which cells are active (cgp_act: inv
// != 0) is one bit per cell, 16 bits per lane, kept in a register from the image's load on.
// The expressions are cgp_apply's (d0 = act ? a0 : 0, its operand order) and, for p = r inv + beta p, x + alpha p, r - alpha q
// and r.(r inv), the table kernel's with inv in place of the table's value; with the same mapping and sum order a system that
// has a dictionary gets the bits of k_cg_image.
//
// Loads: scalar plane base of the image + the lane's 32-bit byte offset, without branches -- a lane beyond the image's last
// pair reads pair 0 instead (its p and r are zeros, its A p is replaced by zeros, its x is not stored), so every wave issues
// the same number of loads and the waits stay counted.  A pair's loads are issued together in front of its LDS reads and
// arithmetic; the rows of pair k + 1 are NOT requested ahead of pair k's arithmetic: a second row set is 20 VGPRs beside q, r
// (64) and a pair's own row and p values, and the lane has 128 -- written that way the kernel spilled 164 B per lane.  The
// compute unit's other 15 waves are what covers a wave's wait.  The loads are ordinary (temporal) ones: unlike the streaming
// form this kernel reads the planes again a few microseconds later (non-temporal loads of the planes: measured, slower).
#pragma once
#include "kernels_cg_image.hpp"
#include "kernels_cg_planes.hpp"

namespace deff {

// the five matrix planes and cg_inv of one image as scalar bases
struct CgpiBase {
    cgp_gptr a0, aW, aE, aS, aN, inv;
};

__device__ __forceinline__ CgpRow cgpi_row(const CgpiBase &B, unsigned off)
{
    CgpRow m;
    m.a0 = cgp_gld2(B.a0, off);
    m.aW = cgp_gld2(B.aW, off);
    m.aE = cgp_gld2(B.aE, off);
    m.aS = cgp_gld2(B.aS, off);
    m.aN = cgp_gld2(B.aN, off);
    return m;
}

// A p of pair j from the row's values: cgi_apply's reads of p (own pair c, the pairs a row up and down, the outer W / E cells
// of lanes 0 / 63 from LDS and those of the others from their neighbouring lanes) and cgp_apply's expressions, one cell after
// the other.  act: bit 0 / 1 = the pair's first / second cell is active.
__device__ __forceinline__ double2 cgpi_apply(const CgpRow &m, unsigned act, const char *pl, int a, int rowb, int endb, int lane,
                                              double2 &c)
{
    c = *reinterpret_cast<const double2 *>(pl + a);
    const int an = a >= rowb ? a - rowb : a, as = a + rowb < endb ? a + rowb : a;
    const double2 n = *reinterpret_cast<const double2 *>(pl + an);
    const double2 s = *reinterpret_cast<const double2 *>(pl + as);
    double h = 0.0;
    if (lane == 0) h = *reinterpret_cast<const double *>(pl + (a > 0 ? a - 8 : a));
    if (lane == 63) h = *reinterpret_cast<const double *>(pl + (a + 16 < endb ? a + 16 : a));
    const double w = dpp_f64_keep<0x138>(c.y, h);               // wave_shr:1, lane 0 keeps its outer neighbour
    const double e = dpp_f64_keep<0x130>(c.x, h);               // wave_shl:1, lane 63 keeps its outer neighbour
    const double d0 = (act & 1u) ? m.a0.x : 0.0, d1 = (act & 2u) ? m.a0.y : 0.0;
    double2 ap;
    ap.x = d0 * c.x + m.aW.x * w + m.aE.x * c.y + m.aS.x * s.x + m.aN.x * n.x;
    ap.y = d1 * c.y + m.aW.y * c.x + m.aE.y * e + m.aS.y * s.y + m.aN.y * n.y;
    return ap;
}

__global__ __launch_bounds__(CGI_THREADS) void k_cgp_image(CgpPlanes A, const double *__restrict__ inv, double *__restrict__ x,
                                                           double *__restrict__ r, double *__restrict__ p,
                                                           CgScal *__restrict__ sc, int nx, int ny, int nimg, long long n_iter,
                                                           double tol2, long long max_iter)
{
    __shared__ __attribute__((aligned(16))) double lds[CGI_CELLS + 3 * CGI_WAVES];
    double(*ws)[CGI_WAVES] = reinterpret_cast<double(*)[CGI_WAVES]>(lds + CGI_CELLS);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    char *pl = reinterpret_cast<char *>(lds);
    const int npairs = nx * ny / 2;                             // nx (the pitch) is even
    const int rowb = nx * 8, endb = npairs * 16;                // bytes of a row / of the image's p

    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        __syncthreads();                                        // the previous image's LDS reads
        CgScal &s = sc[img];
        if (s.done) continue;                                   // frozen image: no writes
        const size_t base = (size_t)img * npairs;
        const double2 *r2 = reinterpret_cast<const double2 *>(r) + base;
        const size_t cell0 = 2 * base;
        const CgpiBase B{cgp_uniform(A.a0 + cell0), cgp_uniform(A.aW + cell0), cgp_uniform(A.aE + cell0),
                         cgp_uniform(A.aS + cell0), cgp_uniform(A.aN + cell0), cgp_uniform(inv + cell0)};
        const cgp_gptr xb = cgp_uniform(x + cell0);
        double2 qv[CGI_K], rv[CGI_K];                           // q = A p from (B) to (C), and r
        unsigned act = 0;                                       // bits 2k, 2k + 1: the cells of pair k are active
        int tj = t;                                             // (not hoisted out of the image loop: see `ta` below)
        asm volatile("" : "+v"(tj));
#pragma unroll
        for (int k = 0; k < CGI_K; ++k) {
            const int j = tj + CGI_THREADS * k;
            const bool v = j < npairs;
            qv[k] = make_double2(0.0, 0.0);
            rv[k] = v ? r2[j] : make_double2(0.0, 0.0);
            const double2 iv = v ? cgp_gld2(B.inv, 16u * (unsigned)j) : make_double2(0.0, 0.0);
            act |= cgp_act(iv) << (2 * k);
            *reinterpret_cast<double2 *>(pl + 16 * j) = v ? (reinterpret_cast<const double2 *>(p) + base)[j] : make_double2(0.0, 0.0);
        }
        double rho = cgi_uniform(s.rho), beta = cgi_uniform(s.beta), alpha = cgi_uniform(s.alpha), rr_s = cgi_uniform(s.rr);
        const double tolbb = cgi_uniform(tol2 * s.bb);
        long long iters = s.iters;
        int done = 0, restart = __builtin_amdgcn_readfirstlane(s.restart);

        for (long long it = 0; it < n_iter && !done; ++it) {
            // the lane's addresses are recomputed in every iteration, as in k_cg_image
            int ta = 16 * t;
            asm volatile("" : "+v"(ta));
            // byte offset of pair k in a plane of the image; pair 0's for a lane beyond the image's end
            auto off_of = [&](int k) -> unsigned {
                const int a = ta + 16 * CGI_THREADS * k;
                return a < endb ? (unsigned)a : 0u;
            };
            // (A) p = z + beta p, in place: a thread touches its own cells only
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                const int a = ta + 16 * CGI_THREADS * k;
                const double2 iv = cgp_gld2(B.inv, off_of(k));
                double2 pn = make_double2(rv[k].x * iv.x, rv[k].y * iv.y);
                if (!restart) {
                    const double2 pp = *reinterpret_cast<const double2 *>(pl + a);
                    pn = make_double2(pn.x + beta * pp.x, pn.y + beta * pp.y);
                }
                *reinterpret_cast<double2 *>(pl + a) = pn;
            }
            __syncthreads();
            // (B) q = A p, p . q
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                const int a = ta + 16 * CGI_THREADS * k;
                const CgpRow m = cgpi_row(B, off_of(k));
                double2 c;
                double2 ap = cgpi_apply(m, act >> (2 * k), pl, a, rowb, endb, lane, c);
                if (a >= endb) ap = make_double2(0.0, 0.0);
                acc += c.x * ap.x + c.y * ap.y;
                qv[k] = ap;
                __builtin_amdgcn_sched_barrier(0);
            }
            const double wp = wave_sum_to_lane63(acc);
            if (lane == 63) ws[0][wave] = wp;
            __syncthreads();
            const double pap = cgi_sum16(ws[0]);
            restart = 0;
            if (pap > 0.0 && pap <= 1.7976931348623157e308) alpha = rho / pap;
            else { alpha = 0.0; done = 3; break; }
            // (C) x += alpha p (in global memory), r -= alpha q; r.z and r.r of the new r.  Own cells only: no neighbour of p
            double rz = 0.0, rr = 0.0;
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                const int a = ta + 16 * CGI_THREADS * k;
                const unsigned off = off_of(k);
                const double2 iv = cgp_gld2(B.inv, off);
                double2 xx = cgp_gld2(xb, off);
                const double2 c = *reinterpret_cast<const double2 *>(pl + a);
                xx.x = xx.x + alpha * c.x;
                xx.y = xx.y + alpha * c.y;
                if (a < endb) cgp_gst2(xb, off, xx);
                rv[k].x = rv[k].x - alpha * qv[k].x;
                rv[k].y = rv[k].y - alpha * qv[k].y;
                rz += rv[k].x * (rv[k].x * iv.x) + rv[k].y * (rv[k].y * iv.y);
                rr += rv[k].x * rv[k].x + rv[k].y * rv[k].y;
                __builtin_amdgcn_sched_barrier(0);
            }
            const double w1 = wave_sum_to_lane63(rz), w2 = wave_sum_to_lane63(rr);
            if (lane == 63) { ws[1][wave] = w1; ws[2][wave] = w2; }
            __syncthreads();
            const double srz = cgi_sum16(ws[1]);
            rr_s = cgi_sum16(ws[2]);
            iters += 1;
            if (rr_s <= tolbb) done = 1;
            else if (iters >= max_iter) done = 2;
            else {
                beta = srz / rho;
                rho = srz;
            }
        }

        asm volatile("" : "+v"(tj));
#pragma unroll
        for (int k = 0; k < CGI_K; ++k) {
            const int j = tj + CGI_THREADS * k;
            if (j < npairs) {
                (reinterpret_cast<double2 *>(r) + base)[j] = rv[k];
                (reinterpret_cast<double2 *>(p) + base)[j] = *reinterpret_cast<const double2 *>(pl + 16 * j);
            }
        }
        if (t == 0) {
            s.rho = rho;
            s.alpha = alpha;
            s.beta = beta;
            s.rr = rr_s;
            s.iters = iters;
            s.done = done;
            s.restart = restart;
        }
    }
}

}  // namespace deff
