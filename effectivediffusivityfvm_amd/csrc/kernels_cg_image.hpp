// kernels_cg_image.hpp -- conjugate gradients of a whole small image on ONE compute unit (tuning key "cg_onchip",
// api_cg.hip; DESIGN.md section 9, "On chip").  The recurrence is that of kernels_cg.hpp (k_cg_dir / k_cg_alpha / k_cg_update /
// k_cg_beta), iteration by iteration; what changes is where the state lives and how the two dot products are summed.
//
// An image of pitch x ny <= 16 384 cells is taken by one workgroup of 1024 threads (16 waves, 128 VGPRs each):
//   LDS        the CG table (28.4 KiB, as the streaming kernels hold it), p (up to 128 KiB) and 3 x 16 wave sums
//   registers  x, r and the 16-bit codes of the lane's 16 cells: pairs j = t + 1024 k, k = 0..7, of the image's flat cell
//              array, i.e. 16-byte slot t of 16 KiB block k -- every ds_read_b128 / ds_write_b128 of a wave is 1 KiB
//              contiguous (conflict-free), and a pair's W / E neighbours are the neighbouring lanes' pairs (DPP; lanes 0
//              and 63 read theirs from LDS), its N / S neighbours the pairs j -+ pitch / 2
// One iteration: (A) p = z + beta p in place | barrier | (B) p.Ap -> wave sums | barrier | alpha; (C) Ap again, x += alpha p,
// r -= alpha Ap, r.z and r.r -> wave sums | barrier | beta or stop.  Nothing leaves the CU between the load of (x, r, p,
// codes) and their store after n iterations or the image's stop.
//
// The flat mapping needs no knowledge of rows: a link that would leave the image (W of the first column, E of the last, N of
// the first row, S of the last) is 0 in every admissible system (k_cg_admissible), so the cell such a link reads -- the end of
// the neighbouring row, or the pair itself where the index would leave the image -- is multiplied by 0.
//
// Determinism: a lane adds its pairs in k order, a wave by wave_sum_to_lane63, every thread the 16 wave sums in wave order;
// none of it depends on the launch (images, workgroups), so an image of a stack gives the bits of a one-image context, and
// a launch of n iterations the bits of n launches of one (all of the state is written back in full precision).
#pragma once
#include "kernels_cg.hpp"

namespace deff {

constexpr int CGI_THREADS = 1024;
constexpr int CGI_WAVES = CGI_THREADS / 64;
constexpr int CGI_K = 8;                                        // cell pairs per lane
constexpr int CGI_CELLS = 2 * CGI_K * CGI_THREADS;              // 16 384: 128 KiB of p

__device__ __forceinline__ double cgi_uniform(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// a value the compiler cannot split or precompute outside the loop it is used in: the two 16-bit codes of a pair stay one
// register, a lane's LDS addresses are recomputed where they are used (hoisted, they are registers the lane does not have)
__device__ __forceinline__ unsigned cgi_opaque(unsigned v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// the 16 wave sums in wave order (every thread, the same bits)
__device__ __forceinline__ double cgi_sum16(const double *ws)
{
    double s = ws[0];
#pragma unroll
    for (int w = 1; w < CGI_WAVES; ++w) s = s + ws[w];
    return cgi_uniform(s);
}

// A p of pair j (byte address a = 16 j of its p in `pl`): own pair c, the pairs a row up and down, the outer W / E cells
// of lanes 0 / 63 from LDS and those of the others from their neighbouring lanes
__device__ __forceinline__ double2 cgi_apply(const double *tab, const char *pl, unsigned cw, int a, int rowb, int endb, int lane,
                                             double2 &c)
{
    c = *reinterpret_cast<const double2 *>(pl + a);
    const int an = a >= rowb ? a - rowb : a, as = a + rowb < endb ? a + rowb : a;
    const double2 n = *reinterpret_cast<const double2 *>(pl + an);
    const double2 s = *reinterpret_cast<const double2 *>(pl + as);
    double h = 0.0;
    if (lane == 0) h = *reinterpret_cast<const double *>(pl + (a > 0 ? a - 8 : a));
    if (lane == 63) h = *reinterpret_cast<const double *>(pl + (a + 16 < endb ? a + 16 : a));
    // cg_apply's expressions, one cell after the other (sched_barrier: with both cells' ten table values in flight the lane
    // runs out of registers)
    const double w = dpp_f64_keep<0x138>(c.y, h);               // wave_shr:1, lane 0 keeps its outer neighbour
    const double e = dpp_f64_keep<0x130>(c.x, h);               // wave_shl:1, lane 63 keeps its outer neighbour
    const unsigned o0 = cw & 0xFFFFu, o1 = cw >> 16;
    double2 ap;
    ap.x = cg_v<CG_A0>(tab, o0) * c.x + cg_v<CG_W>(tab, o0) * w + cg_v<CG_E>(tab, o0) * c.y + cg_v<CG_S>(tab, o0) * s.x +
           cg_v<CG_N>(tab, o0) * n.x;
    __builtin_amdgcn_sched_barrier(0);
    ap.y = cg_v<CG_A0>(tab, o1) * c.y + cg_v<CG_W>(tab, o1) * c.x + cg_v<CG_E>(tab, o1) * e + cg_v<CG_S>(tab, o1) * s.y +
           cg_v<CG_N>(tab, o1) * n.y;
    return ap;
}

__global__ __launch_bounds__(CGI_THREADS) void k_cg_image(const double *__restrict__ tab_g, int nrows,
                                                          const uint16_t *__restrict__ code, double *__restrict__ x,
                                                          double *__restrict__ r, double *__restrict__ p,
                                                          CgScal *__restrict__ sc, int nx, int ny, int nimg, long long n_iter,
                                                          double tol2, long long max_iter)
{
    // one array, the table first: its plane offsets then fit the 16-bit offset field of the LDS instructions
    __shared__ __attribute__((aligned(16))) double lds[CG_DOUBLES + CGI_CELLS + 3 * CGI_WAVES];
    double *tab = lds, (*ws)[CGI_WAVES] = reinterpret_cast<double (*)[CGI_WAVES]>(lds + CG_DOUBLES + CGI_CELLS);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    for (int k = t; k < CG_PLANES * nrows; k += CGI_THREADS) {
        const int pl = k / nrows, row = k - pl * nrows;
        tab[pl * LUT_PLANE_STRIDE + row] = tab_g[pl * LUT_PLANE_STRIDE + row];
    }
    char *pl = reinterpret_cast<char *>(lds + CG_DOUBLES);
    const int npairs = nx * ny / 2;                             // nx (the pitch) is even
    const int rowb = nx * 8, endb = npairs * 16;                // bytes of a row / of the image's p

    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        __syncthreads();                                        // the table; the previous image's LDS reads
        CgScal &s = sc[img];
        if (s.done) continue;                                   // frozen image: no writes
        const size_t base = (size_t)img * npairs;
        const double2 *x2 = reinterpret_cast<const double2 *>(x) + base, *r2 = reinterpret_cast<const double2 *>(r) + base;
        const unsigned *c2 = reinterpret_cast<const unsigned *>(code) + base;
        double2 xv[CGI_K], rv[CGI_K];
        unsigned cw[CGI_K];
        int tj = t;                                             // (not hoisted out of the image loop: see `ta` below)
        asm volatile("" : "+v"(tj));
#pragma unroll
        for (int k = 0; k < CGI_K; ++k) {
            const int j = tj + CGI_THREADS * k;
            const bool v = j < npairs;
            xv[k] = v ? x2[j] : make_double2(0.0, 0.0);
            rv[k] = v ? r2[j] : make_double2(0.0, 0.0);
            cw[k] = v ? c2[j] : 0u;                             // code 0: the zero row
            *reinterpret_cast<double2 *>(pl + 16 * j) = v ? (reinterpret_cast<const double2 *>(p) + base)[j] : make_double2(0.0, 0.0);
        }
        double rho = cgi_uniform(s.rho), beta = cgi_uniform(s.beta), alpha = cgi_uniform(s.alpha), rr_s = cgi_uniform(s.rr);
        const double tolbb = cgi_uniform(tol2 * s.bb);
        long long iters = s.iters;
        int done = 0, restart = __builtin_amdgcn_readfirstlane(s.restart);

        for (long long it = 0; it < n_iter && !done; ++it) {
            // the lane's LDS addresses are recomputed in every iteration (a few VALU operations per pair): hoisted out of the
            // loop they would be 40 registers the lane does not have
            int ta = 16 * t;
            asm volatile("" : "+v"(ta));
            // (A) p = z + beta p, in place: a thread touches its own cells only
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                const int a = ta + 16 * CGI_THREADS * k;
                const unsigned cwk = cgi_opaque(cw[k]);
                double2 pn = make_double2(rv[k].x * cg_v<CG_INV>(tab, cwk & 0xFFFFu), rv[k].y * cg_v<CG_INV>(tab, cwk >> 16));
                if (!restart) {
                    const double2 pp = *reinterpret_cast<const double2 *>(pl + a);
                    pn = make_double2(pn.x + beta * pp.x, pn.y + beta * pp.y);
                }
                *reinterpret_cast<double2 *>(pl + a) = pn;
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            // (B) p . A p
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                double2 c;
                const unsigned cwk = cgi_opaque(cw[k]);
                const double2 ap = cgi_apply(tab, pl, cwk, ta + 16 * CGI_THREADS * k, rowb, endb, lane, c);
                acc += c.x * ap.x + c.y * ap.y;
                __builtin_amdgcn_sched_barrier(0);
            }
            const double wp = wave_sum_to_lane63(acc);
            if (lane == 63) ws[0][wave] = wp;
            __syncthreads();
            const double pap = cgi_sum16(ws[0]);
            restart = 0;
            if (pap > 0.0 && pap <= 1.7976931348623157e308) alpha = rho / pap;
            else { alpha = 0.0; done = 3; break; }
            // (C) x += alpha p, r -= alpha A p; r.z and r.r of the new r
            double rz = 0.0, rr = 0.0;
#pragma unroll
            for (int k = 0; k < CGI_K; ++k) {
                if (CGI_THREADS * k + 64 * wave >= npairs) break;
                double2 c;
                const unsigned cwk = cgi_opaque(cw[k]);
                const double2 ap = cgi_apply(tab, pl, cwk, ta + 16 * CGI_THREADS * k, rowb, endb, lane, c);
                xv[k].x = xv[k].x + alpha * c.x;
                xv[k].y = xv[k].y + alpha * c.y;
                asm volatile("" : "+v"(xv[k].x), "+v"(xv[k].y));    // here, not sunk to the loop's end with c kept alive
                rv[k].x = rv[k].x - alpha * ap.x;
                rv[k].y = rv[k].y - alpha * ap.y;
                rz += rv[k].x * (rv[k].x * cg_v<CG_INV>(tab, cwk & 0xFFFFu)) + rv[k].y * (rv[k].y * cg_v<CG_INV>(tab, cwk >> 16));
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
                (reinterpret_cast<double2 *>(x) + base)[j] = xv[k];
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
