// kernels_tb.hpp -- matrix-free sweeps with temporal blocking: T weighted-Jacobi
// sweeps per pass over HBM (gfx950, wave64, FP64).
//
// Legal because the reference only inspects the field every 10 000 sweeps
// (Deff2DGPU/Deff2D.cuh:1243); each of the T sweeps is the same updateX_SOR
// arithmetic (cuh:69-92) as the single-sweep kernels, so results stay
// bit-identical -- a cell's value after sweep k does not depend on which kernel
// produced it.
//
// Structure: every WAVE is independent.  A wave owns a strip of 128 columns
// (2 per lane) and streams down the rows of its chunk.  Per input row it
//   level 0   loads the row of x (16 B per lane, coalesced) and its row codes (4 B per lane),
//   level t   (t = 1..T) computes row r-t of sweep t from the three newest rows
//             of sweep t-1, all held in registers (a 3-row window per level);
//             W/E neighbours come from the adjacent lanes by DPP wave shifts,
//             N/S from the window; coefficients from the row dictionary in LDS,
//   level T   is stored (16 B per lane).
// After t sweeps the outermost t columns/rows of a strip are stale, so a strip
// produces 128 - 2T valid columns and needs T extra rows above and below its
// chunk: neighbouring strips overlap by 2T and recompute the overlap instead of
// synchronising.  No barrier, no inter-wave traffic inside the row loop.
//
// HBM traffic per cell per sweep: (8 + 2) / T / efficiency read + 8 / T
// written -- 2.7 B measured at T = 8 against 18 B for the single-sweep
// matrix-free kernel and 64 B for explicit coefficients; the kernel is bound by
// how many waves of a SIMD are ready to issue FP64 (SQ counters: VALU ~50-60 % busy, LDS ~40 %;
// see the notes at tb_strip and DESIGN.md section 4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_sweep.hpp"

namespace deff {

constexpr int TB_COLS = 128;                                   // columns per wave strip (2 per lane)
template <bool V> struct TbTag { static constexpr bool value = V; };   // compile-time flag for generic lambdas
template <int V> struct TbInt { static constexpr int value = V; };     // compile-time index for generic lambdas
// f(TbInt<G>{}) for G = FIRST ... N - 1, in order, until one returns false: straight-line code with one exit per call
template <int FIRST, int N, class F> __device__ __forceinline__ void tb_each_until(F &&f)
{
    if constexpr (FIRST < N) {
        if (f(TbInt<FIRST>{})) tb_each_until<FIRST + 1, N>(f);
    }
}
// diagnostics of the chained kernel (tools/tb_stamps.py --chain): wall clocks taken inside tb_strip, kept in scalar registers
struct TbMarks {
    unsigned long long first_row, steady;          // first row consumed; entry into the steady-state loop
};

// lane i <- lane i-1 (lane 0 <- 0.0)
__device__ __forceinline__ double from_lane_below(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);   // bound_ctrl: lane 0 <- 0
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i+1 (lane 63 <- 0.0)
__device__ __forceinline__ double from_lane_above(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// One cell.  `off` is the cell's code: the BYTE offset of its row in plane 0 of the row
// dictionary (lut_layout.hpp); the other planes sit at fixed strides.
// GUARD = reference's non-zero test on every link (needed when a phase has zero
// diffusivity: links are -0.0 and neighbours may hold NaN/Inf, cuh:77).  Without
// it a zero link multiplies a finite value and adds +-0, which leaves sigma
// unchanged, so both forms give the same bits.  WALL = the strip contains the
// first or last column; everywhere else b is identically +0.0 and its lookup is
// skipped (0.0 - sigma is still evaluated as a subtraction, so the bits match).
template <bool GUARD, bool WALL, bool FMA>
__device__ __forceinline__ double tb_cell(const double *lut, unsigned off, double xc, double xw, double xe,
                                          double xs, double xn, double omw)
{
    const char *base = reinterpret_cast<const char *>(lut) + off;
    constexpr int PS = LUT_PLANE_STRIDE * 8;
    const double c0 = *reinterpret_cast<const double *>(base);
    const double aW = *reinterpret_cast<const double *>(base + PS);
    const double aE = *reinterpret_cast<const double *>(base + 2 * PS);
    const double aS = *reinterpret_cast<const double *>(base + 3 * PS);
    const double aN = *reinterpret_cast<const double *>(base + 4 * PS);
    double b = 0.0;
    if constexpr (WALL) b = *reinterpret_cast<const double *>(base + 5 * PS);
    if constexpr (GUARD) {
        return jacobi_cell<FMA>(c0, aW, aE, aS, aN, b, xc, xw, xe, xs, xn, omw);
    } else {
        // the reference starts from sigma = 0 (cuh:74); 0 + p differs from p only in the sign of a
        // zero, which b - sigma cannot see (b is +0 or non-zero), so the leading add is dropped
        // (in the contracted form the first term is fma(aW, xw, 0) = the rounded product, likewise)
        double sigma = aW * xw;
        sigma = mul_add<FMA>(aE, xe, sigma);
        sigma = mul_add<FMA>(aS, xs, sigma);
        sigma = mul_add<FMA>(aN, xn, sigma);
        if constexpr (FMA) return __builtin_fma(omw, xc, c0 * (b - sigma));
        else return omw * xc + c0 * (b - sigma);
    }
}

// The two cells of a lane TOGETHER, one arithmetic stage at a time: cell by cell (two tb_cell() calls) hipcc emits each
// cell's seven-deep dependent chain back to back, so that a wave has a single chain in flight; written stage-wise the two
// chains interleave and every FP64 instruction has another between itself and its consumer.  Same operations, same order
// per cell, same bits.
// the matrix rows of a lane's two cells
constexpr int TB_STAGE_FENCE = 0x4;                             // sched_barrier mask: SALU may cross, nothing else
struct TbCoef {
    double c0[2], aW[2], aE[2], aS[2], aN[2], b[2];
};
// PRE = the pre-scaled table (kernels_sweep.hpp, pre_cell): plane 0 is not read, b' comes first because the chain starts with it
template <bool WALL, bool PRE = false>
__device__ __forceinline__ void tb_lookup(const double *lut, unsigned o0, unsigned o1, TbCoef &k)
{
    constexpr int PS = LUT_PLANE_STRIDE * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const char *base = reinterpret_cast<const char *>(lut) + (h ? o1 : o0);
        if constexpr (PRE) {
            if constexpr (WALL) k.b[h] = *reinterpret_cast<const double *>(base + 5 * PS);
            else k.b[h] = 0.0;
        }
        k.aW[h] = *reinterpret_cast<const double *>(base + PS);
        k.aE[h] = *reinterpret_cast<const double *>(base + 2 * PS);
        k.aS[h] = *reinterpret_cast<const double *>(base + 3 * PS);
        k.aN[h] = *reinterpret_cast<const double *>(base + 4 * PS);
        if constexpr (!PRE) {
            k.c0[h] = *reinterpret_cast<const double *>(base);
            if constexpr (WALL) k.b[h] = *reinterpret_cast<const double *>(base + 5 * PS);
            else k.b[h] = 0.0;
        }
    }
}
// The pre-scaled arithmetic of a lane's two cells, stage-wise like tb_apply below: five stages of two independent FMAs, so
// that each FMA has the other cell's between itself and its consumer.  A strip without a wall column passes b' = +0.0 (the
// table's value there: the host looks every row up otherwise, upload_lut_pre), still through an FMA -- fma(omw, x, +0.0)
// is not the bare product when that is -0.0.
template <bool PINNED = false>
__device__ __forceinline__ double2 tb_apply_pre(const TbCoef &k, double2 vC, double xw0, double xe1, double2 vS, double2 vN, double omw)
{
    auto stage = []() __attribute__((always_inline)) {
        if constexpr (PINNED) __builtin_amdgcn_sched_barrier(TB_STAGE_FENCE);
    };
    double s0 = __builtin_fma(omw, vC.x, k.b[0]), s1 = __builtin_fma(omw, vC.y, k.b[1]);
    stage();
    s0 = __builtin_fma(-k.aW[0], xw0, s0); s1 = __builtin_fma(-k.aW[1], vC.x, s1);
    stage();
    s0 = __builtin_fma(-k.aE[0], vC.y, s0); s1 = __builtin_fma(-k.aE[1], xe1, s1);
    stage();
    s0 = __builtin_fma(-k.aS[0], vS.x, s0); s1 = __builtin_fma(-k.aS[1], vS.y, s1);
    stage();
    double2 o;
    o.x = __builtin_fma(-k.aN[0], vN.x, s0); o.y = __builtin_fma(-k.aN[1], vN.y, s1);
    return o;
}
// PINNED = the stages stay in the order written (a fence between them that only scalar instructions may cross): see tb_strip
template <bool FMA, bool PINNED = false>
__device__ __forceinline__ double2 tb_apply(const TbCoef &k, double2 vC, double xw0, double xe1, double2 vS, double2 vN, double omw)
{
    auto stage = []() __attribute__((always_inline)) {
        if constexpr (PINNED) __builtin_amdgcn_sched_barrier(TB_STAGE_FENCE);
    };
    double s0 = k.aW[0] * xw0, s1 = k.aW[1] * vC.x;
    stage();
    s0 = mul_add<FMA>(k.aE[0], vC.y, s0); s1 = mul_add<FMA>(k.aE[1], xe1, s1);
    stage();
    s0 = mul_add<FMA>(k.aS[0], vS.x, s0); s1 = mul_add<FMA>(k.aS[1], vS.y, s1);
    stage();
    s0 = mul_add<FMA>(k.aN[0], vN.x, s0); s1 = mul_add<FMA>(k.aN[1], vN.y, s1);
    stage();
    s0 = k.b[0] - s0; s1 = k.b[1] - s1;
    stage();
    double2 o;
    if constexpr (FMA) {
        s0 = k.c0[0] * s0; s1 = k.c0[1] * s1;
        stage();
        o.x = __builtin_fma(omw, vC.x, s0); o.y = __builtin_fma(omw, vC.y, s1);
    } else {
        const double m0 = omw * vC.x, m1 = omw * vC.y;
        s0 = k.c0[0] * s0; s1 = k.c0[1] * s1;
        stage();
        o.x = m0 + s0; o.y = m1 + s1;
    }
    return o;
}
template <bool GUARD, bool WALL, bool FMA>
__device__ __forceinline__ double2 tb_pair(const double *lut, unsigned o0, unsigned o1, double2 vC, double xw0, double xe1,
                                           double2 vS, double2 vN, double omw)
{
    if constexpr (GUARD) {
        double2 o;
        o.x = tb_cell<GUARD, WALL, FMA>(lut, o0, vC.x, xw0, vC.y, vS.x, vN.x, omw);
        o.y = tb_cell<GUARD, WALL, FMA>(lut, o1, vC.y, vC.x, xe1, vS.y, vN.y, omw);
        return o;
    } else {
        TbCoef k;
        tb_lookup<WALL>(lut, o0, o1, k);
        return tb_apply<FMA>(k, vC, xw0, xe1, vS, vN, omw);
    }
}


// Raw buffer access to the rows (see tb_strip).  A lane offset of TB_LANE_OUT lies beyond every descriptor: the host only
// launches chunks whose window -- (rows + 2 T) rows of nx doubles -- stays below 2 GiB (tb_window_fits, checked by
// plan_streaming), so every in-range offset, lane part plus row part, is below it and 32-bit offset arithmetic cannot wrap.
typedef unsigned int tb_u4 __attribute__((ext_vector_type(4)));
constexpr unsigned TB_LANE_OUT = 0x80000000u;
constexpr bool tb_window_fits(int nx, int rows, int T)
{
    return ((long long)rows + 2 * T) * nx * 8 < (long long)TB_LANE_OUT;
}
template <class P> __device__ __forceinline__ __amdgpu_buffer_rsrc_t tb_rsrc(P *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(static_cast<const void *>(p)), 0, (int)bytes, 0x00020000);
}

// One strip x chunk: the whole row pipeline of a wave (2 cells per lane, 128 columns).
// Geometry (array rows): the mesh of this image is rows [row_lo, row_lo+ny) -- rows outside it
// are "outside the mesh" even if another image of a batch lives there, and row_lo is negative
// for a row slab whose array is a window into a taller image; the chunk computes rows
// [ry0, min(ry0+LY, own_hi)), own_hi being the end of the rows this launch owns (the image in a
// batch, the slab's own rows -- without its halo -- in a multi-GPU run).
// The code is deliberately written with double2 values and named slots: an array-of-scalars formulation of the same
// dataflow made hipcc hoist the lookups to 204 VGPRs.  Everything that was measured on this function and dropped --
// pipelined lookups, 4 cells per lane, skewed levels, cooperating strips, one lookup per face, LDS-DMA prefetch, fences
// elsewhere, a pair of waves per tile -- is recorded with its numbers in DESIGN.md section 4 and
// profiles/r03_tb_ab_kbench.log; the variants themselves are tools/experiments/r03_tb_variants.patch.
// XAUX = the cache-policy (aux) bits of the x-row accesses -- the row loads of the prologue and of the loop, and the xnew
// stores; 0 = plain (k_sweep_matfree_tb), 16 = sc1 (device-coherent: k_sweep_matfree_tb_chain, whose tiles read their
// neighbours' rows of the same launch).  The code loads stay plain.  In the one-pass kernel sc1 rows measured -0.3 +- 0.3 us
// per 107 us launch: profiles/r06_tb_chain_ab.log.
// `marks` (chained kernel only): two wall clocks for the tile stamps, read into scalar registers where they are taken.
// (measurement switch: -DTB_STRAIGHT_RAMP=0 builds every tile with the generic trimmed groups, to be timed against the default
// build in one process; never set by the Makefile)
#ifndef TB_STRAIGHT_RAMP
#define TB_STRAIGHT_RAMP 1
#endif
// RAMP = full-halo tiles cross their first steps as straight-line code (below).  Off in the loop over the tiles of a workgroup
// that was dealt none (k_sweep_matfree_tb without a table): what the previous tile left in flight would reach this tile's
// steady-state loop along the edge described below.
// PRE = the pre-scaled arithmetic (kernels_sweep.hpp, pre_cell) on the pre-scaled table: same rows, same codes, same pipeline;
// a level is 10 lookups and five stages of two FMAs.  Unguarded tables only.
template <int T, bool GUARD, bool WALL, bool FMA, int XAUX = 0, bool RAMP = true, bool PRE = false>
__device__ __forceinline__ void tb_strip(const double *lut, const uint16_t *__restrict__ code,
                                         const double *__restrict__ x, double *__restrict__ xnew, int nx,
                                         int ny, int row_lo, int own_hi, int tx, int ntx, int shift, int ry0, int LY,
                                         int lane, double omw, TbMarks *marks = nullptr)
{
    static_assert(!(PRE && GUARD), "the pre-scaled form has no guarded variant");
    // column halo rounded up to even so that odd T keeps the 16-B alignment of a lane's pair
    constexpr int HW = (T + 1) & ~1;
    constexpr int WOUT = TB_COLS - 2 * HW;
    // Strip tx reads columns [tx*WOUT, tx*WOUT + 128) and owns the outputs [out_lo, out_hi): its
    // window minus HW stale columns on each side that borders another strip -- a side that is a
    // wall of the mesh needs no halo, so the first strip starts at column 0 and an image of up to
    // 128 columns is a single strip with nothing recomputed.
    // (shift = HW selects the older placement with a halo also outside the first column; kept as
    // a tuning switch so that the two can be compared inside one process.)
    const int col = tx * WOUT - shift + 2 * lane;  // this lane's first column (even)
    const bool in_x = col >= 0 && col < nx;        // nx even => col+1 < nx too
    const int out_lo = (tx == 0) ? 0 : tx * WOUT - shift + HW;
    const int out_hi = (tx == ntx - 1) ? nx : tx * WOUT - shift + TB_COLS - HW;
    const int row_hi = row_lo + ny;
    const int ry1 = min(ry0 + LY, own_hi);
    // input rows [r_begin, r_end): T rows of halo above and below the chunk, except that nothing
    // lies above the first row of the mesh (the steps for rows below the last one still run: they
    // drain the pipeline)
    const int r_begin = max(ry0 - T, row_lo), r_end = ry1 + T;
    const bool st_x = in_x && (col >= out_lo) && (col < out_hi);
    const double2 zero = make_double2(0.0, 0.0);

    // Rows travel through raw buffer descriptors: address = descriptor base (this wave's window, a wave-uniform 64-bit add)
    // + lane offset (one loop-invariant VGPR per array) + row offset (an SGPR).  The hardware's range check does the masking:
    // a lane outside the mesh (loads) or outside [out_lo, out_hi) (stores) carries TB_LANE_OUT, beyond the end of any window,
    // and a row outside the window takes a descriptor of zero bytes (at row offset 0) -- such loads return 0 for x and for the
    // codes, such stores are dropped.  No per-lane 64-bit address, no select, no branch around a store; an address outside
    // the window cannot be formed.  The windows: x and the codes, rows [r_begin, min(r_end, row_hi)); xnew, rows [ry0, ry1).
    const int win_hi = min(r_end, row_hi);
    const unsigned xrow = (unsigned)nx * 8u, crow = (unsigned)nx * 2u;                 // bytes per row (tb_window_fits: no overflow below)
    const unsigned lrows = (unsigned)max(win_hi - r_begin, 0), srows = (unsigned)max(ry1 - ry0, 0);
    const double *const xwin = x + (ptrdiff_t)r_begin * nx;
    const uint16_t *const cwin = code + (ptrdiff_t)r_begin * nx;
    double *const swin = xnew + (ptrdiff_t)ry0 * nx;
    const unsigned vo_x = in_x ? (unsigned)col * 8u : TB_LANE_OUT;
    const unsigned vo_c = in_x ? (unsigned)col * 2u : TB_LANE_OUT;
    const unsigned vo_s = st_x ? (unsigned)col * 8u : TB_LANE_OUT;

    double2 w[T][3];                               // w[t]: 3 newest rows of sweep t
    unsigned cw[T + 1];                            // cw[t]: the two 16-bit codes of row rr-t
                                                   // (both zeroed where the generic trimmed groups start, see below)

    // (rr >= r_begin for every row asked for: the loops below start there and only go down)
    auto fetch = [&](const int rr, tb_u4 &vx_out, unsigned &vc_out) __attribute__((always_inline)) {
        const bool ok = rr < win_hi;                                                  // wave-uniform
        const unsigned k = ok ? (unsigned)(rr - r_begin) : 0u;
        vx_out = __builtin_amdgcn_raw_buffer_load_b128(tb_rsrc(xwin, ok ? lrows * xrow : 0u), (int)vo_x, (int)(k * xrow), XAUX);
        vc_out = __builtin_amdgcn_raw_buffer_load_b32(tb_rsrc(cwin, ok ? lrows * crow : 0u), (int)vo_c, (int)(k * crow), 0);
    };
    auto store = [&](const int rt, const double2 o) __attribute__((always_inline)) {
        const bool go = rt >= ry0 && rt < ry1;                                        // wave-uniform
        const unsigned k = go ? (unsigned)(rt - ry0) : 0u;
        tb_u4 v;
        __builtin_memcpy(&v, &o, 16);
        __builtin_amdgcn_raw_buffer_store_b128(v, tb_rsrc(swin, go ? srows * xrow : 0u), (int)vo_s, (int)(k * xrow), XAUX);
    };
    // Three rows are always in flight: row rr + 3 is asked for at the top of the step that consumes row rr, into the
    // registers that row has just left (nx_*[rr % 3 by position in the group]).
    tb_u4 nx_x[3];                                 // (kept as loaded, 16 bytes: two doubles)
    unsigned nx_c[3];
    // (the first three rows are requested where the steps begin, below)

    // One level of one step: row rt of sweep t from the three newest rows of sweep t - 1 (window slots sN, sC, sS).
    auto level = [&](const int t, const int rt, const int sN, const int sC, const int sS) __attribute__((always_inline)) {
        const double2 vN = w[t - 1][sN], vC = w[t - 1][sC], vS = w[t - 1][sS];
        const double xw0 = from_lane_below(vC.y);
        const double xe1 = from_lane_above(vC.x);
        const unsigned o0 = cw[t] & 0xFFFFu, o1 = cw[t] >> 16;
        double2 o;
        if constexpr (GUARD) {
            o = tb_pair<GUARD, WALL, FMA>(lut, o0, o1, vC, xw0, xe1, vS, vN, omw);
        } else {
            // The lookups first, then the arithmetic stage by stage, both cells side by side, as written: left to
            // itself inside a level the scheduler -- short of registers at 3 waves per SIMD -- runs one cell's chain
            // to its end before it starts the other's (each FP64 instruction then waits for the one before it).
            // That it did not do so before was an accident of a register pressure ABOVE the budget, which made it
            // give the schedule up and keep the source order; the fences say it.
            TbCoef k;
            tb_lookup<WALL, PRE>(lut, o0, o1, k);
            __builtin_amdgcn_sched_barrier(TB_STAGE_FENCE);
            if constexpr (PRE) o = tb_apply_pre<true>(k, vC, xw0, xe1, vS, vN, omw);
            else o = tb_apply<FMA, true>(k, vC, xw0, xe1, vS, vN, omw);
        }
        if (t < T) w[t][sS] = o;
        else store(rt, o);
        // keep the scheduler from pulling the next sweeps' table lookups up here: left
        // alone it hoists them all (180-250 VGPRs, 1-2 waves per SIMD); with the fence a
        // step keeps ~120 VGPRs and 4 waves per SIMD hide the LDS latency instead
        __builtin_amdgcn_sched_barrier(0);
    };
    // A requested row enters the window (slot sS of level 0) and its codes cw[0]: see the comment in `group`.
    auto take = [&](const tb_u4 &vx, const unsigned vc, const int sS) __attribute__((always_inline)) {
        double lo, hi;
        __builtin_memcpy(&lo, &vx, 8);
        __builtin_memcpy(&hi, reinterpret_cast<const char *>(&vx) + 8, 8);
        asm volatile("v_mov_b64 %0, %3\n\tv_mov_b64 %1, %4\n\tv_mov_b32 %2, %5"
                     : "=&v"(w[0][sS].x), "=&v"(w[0][sS].y), "=&v"(cw[0])
                     : "v"(lo), "v"(hi), "v"(vc));
    };
    // (Measured with the tile time stamps, tools/tb_stamps.py: waves sharing a SIMD are served oldest-first, so identical
    // tiles end at 71 / 89 / 108 us of one T = 8 launch at 4096^2, by wave slot.  Evening that out with s_setprio -- a
    // rotating priority per group of steps -- brought +2...4 %: served in turn the three waves issue less in total than served
    // oldest-first.  What is kept is the other way round: the service order stays and the TILES differ, the oldest wave of a
    // SIMD getting the tallest chunk -- `dealt` below, deal_ranked_tiles in api_sweep.hip: +6...8 %.)
    // One group of three steps (input rows r, r+1, r+2).  TRIM = the group may contain levels whose
    // output row this chunk does not need: sweep t needs rows from max(mesh top, ry0 - (T - t)) on, and
    // produces row rr - t at the step that reads row rr, so for the first 2T steps of a chunk (T at the
    // top of the mesh) part of the levels would only compute rows nothing reads -- 72 of 528 level
    // steps at T = 8 with 50-row chunks.  The trimmed groups skip them behind wave-uniform branches;
    // the steady-state loop below stays branch-free (a branch around every level of every step was
    // measured 8 % slower).  A skipped level leaves its window slot as it was: finite values that are
    // read only through zero links or not at all.
    auto group = [&](const int r, auto trim_tag) __attribute__((always_inline)) {
        constexpr bool TRIM = decltype(trim_tag)::value;
#pragma unroll
        for (int ph = 0; ph < 3; ++ph) {
            const int rr = r + ph;                 // input row of this step
            // after this step's level-(t-1) write: newest = slot ph, previous = (ph+2)%3, oldest = (ph+1)%3
            const int sN = (ph + 1) % 3, sC = (ph + 2) % 3, sS = ph;
#pragma unroll
            for (int t = T; t >= 1; --t) cw[t] = cw[t - 1];
            // Row rr, asked for three steps ago, is consumed HERE, behind the previous step's last level fence, by register moves
            // the compiler cannot place elsewhere or fold away (moves, not loads: the loads stay the compiler's, and so does
            // counting them).  Written as plain copies, the copies are coalesced with the loop-carried registers: hipcc then
            // copies the loaded rows at the loop's end, or inside level 1 of the next step, and waits for loads it issued one
            // step or ~50 instructions earlier.  CDNA counts loads and stores in one vmcnt, in issue order; with no branch in
            // the loop the compiler knows what is in flight and waits in front of these moves with a counted vmcnt(4...6): rows
            // rr + 1 and rr + 2 and the stores of the last two steps stay in flight.  tests/test_tb_stream_isa.py holds the
            // emitted loop to that: one branch, no wait that forces a store younger than one step (none with vmcnt 0), first
            // read of a row at least two steps after its load, no select, no 64-bit address arithmetic.
            take(nx_x[ph], nx_c[ph], sS);
            fetch(rr + 3, nx_x[ph], nx_c[ph]);
#pragma unroll
            for (int t = 1; t <= T; ++t) {
                const int rt = rr - t;             // row produced by sweep t in this step
                if constexpr (TRIM) {
                    if (rt < row_lo || rt - t < ry0 - T) {   // wave-uniform: above the mesh / above this level's halo
                        __builtin_amdgcn_sched_barrier(0);
                        continue;
                    }
                }
                level(t, rt, sN, sC, sS);
            }
        }
    };
    constexpr int TRIMMED = ((2 * T + 2) / 3) * 3;   // steps that may hold unneeded levels, rounded up to whole groups
    int r = r_begin;
    if constexpr (!(RAMP && TB_STRAIGHT_RAMP)) {
        // every tile through the generic trimmed groups
#pragma unroll
        for (int t = 0; t < T; ++t) { w[t][0] = zero; w[t][1] = zero; w[t][2] = zero; }
#pragma unroll
        for (int t = 0; t <= T; ++t) cw[t] = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) fetch(r_begin + k, nx_x[k], nx_c[k]);
        if (marks) marks->first_row = wall_clock64();                                  // (here: in front of the first group)
        for (; r < r_begin + TRIMMED && r < r_end; r += 3) group(r, TbTag<true>{});
    } else if (r >= r_end) {
        return;                                    // no input row: an empty chunk
    } else if (ry0 - T >= row_lo && r_end - r_begin > TRIMMED - 3) {
        // The ramp of a tile whose window starts a full halo above its chunk -- every chunk but the topmost of a mesh: step j
        // (input row r_begin + j) needs exactly the levels 1 ... j / 2 (the test of the trimmed groups, rt - t >= ry0 - T, with
        // r_begin = ry0 - T), known when the code is written.  So the same TRIMMED steps are straight-line code: no branch
        // around a level, no window slot zeroed -- level t first runs at step 2 t, when steps 2 t - 2 ... 2 t have written the
        // three rows it reads -- and no test between the groups either: a chunk of one row already has 2 T + 1 input rows,
        // more than TRIMMED - 3, so the loop over the trimmed groups runs them all (the second condition above says so for
        // every T; a chunk too short for it, which no caller sends, would take the generic groups).  One basic block: the
        // requests stay where they are written.
        // And while the upper levels' windows are dead their registers hold rows: the prologue asks for RAMP_ROWS rows at
        // once, steps 0, 1, 2 for three more, and the wave crosses the ramp -- a step holds few levels, a fraction of a
        // memory round trip -- in one or two round trips of the device-coherent rows instead of one per group.  From row
        // RAMP_ROWS on the rows travel as in the loop, three steps ahead through nx_*, which the loop finds as it expects them:
        // rows r, r + 1, r + 2 of its first group in nx_*[0...2].  All requests go through `fetch`: inside the window, or
        // answered by the descriptor of zero bytes.
        constexpr int RAMP_ROWS = TRIMMED - 3 < 3 ? 3 : TRIMMED - 3 > 12 ? 12 : TRIMMED - 3;   // (T = 8: 12 of the 18; a multiple of 3)
        constexpr int NEX = RAMP_ROWS > 3 ? RAMP_ROWS - 3 : 1;
        tb_u4 ex_x[NEX];                           // rows 3 ... RAMP_ROWS - 1 of the window, as loaded
        unsigned ex_c[NEX];
        tb_each_until<0, RAMP_ROWS>([&](auto k_tag) __attribute__((always_inline)) {
            constexpr int k = decltype(k_tag)::value;
            if constexpr (k < 3) fetch(r_begin + k, nx_x[k], nx_c[k]);
            else fetch(r_begin + k, ex_x[k - 3], ex_c[k - 3]);
            return true;
        });
        auto ramp_step = [&](auto j_tag) __attribute__((always_inline)) {
            constexpr int j = decltype(j_tag)::value, ph = j % 3;
            constexpr int sN = (ph + 1) % 3, sC = (ph + 2) % 3, sS = ph;
            const int rr = r_begin + j;
#pragma unroll
            for (int t = T; t >= 1; --t) cw[t] = cw[t - 1];
            if constexpr (j >= 3 && j < RAMP_ROWS) take(ex_x[j - 3], ex_c[j - 3], sS);
            else take(nx_x[ph], nx_c[ph], sS);
            if constexpr (j < 3) fetch(rr + RAMP_ROWS, nx_x[ph], nx_c[ph]);
            else if constexpr (j >= RAMP_ROWS) fetch(rr + 3, nx_x[ph], nx_c[ph]);
            if constexpr (j == 0) {
                if (marks) marks->first_row = wall_clock64();
            }
            tb_each_until<1, (j / 2 < T ? j / 2 : T) + 1>([&](auto t_tag) __attribute__((always_inline)) {
                constexpr int t = decltype(t_tag)::value;
                level(t, rr - t, sN, sC, sS);
                return true;
            });
        };
        tb_each_until<0, TRIMMED>([&](auto j_tag) __attribute__((always_inline)) {
            ramp_step(j_tag);
            return true;
        });
        r += TRIMMED;
    } else {
        // the top of a mesh (the first chunk of an image -- of every image of a stack -- and a slab whose window is clipped):
        // which levels a step needs depends on where the mesh begins; skipped levels leave their slots as they are, zero
        // (Both arms begin by requesting row r_begin, and the compiler lifts what they share in front of the branch.  The
        // emitted control flow has an edge from there straight to the steady-state loop -- never taken, but the loop's waits
        // are counted along it too, and a request in flight on it means vmcnt(0) in every round.  No load is lifted across
        // this line.  For the same reason a caller must not arrive here with operations in flight that the compiler knows
        // of: see RAMP.)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t = 0; t < T; ++t) { w[t][0] = zero; w[t][1] = zero; w[t][2] = zero; }
#pragma unroll
        for (int t = 0; t <= T; ++t) cw[t] = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) fetch(r_begin + k, nx_x[k], nx_c[k]);
        if (marks) marks->first_row = wall_clock64();                                  // (here: in front of the first group)
        // (at least one group, as tested above: no way from the requests just made straight to the loop below, which would
        // then have to wait for them in every round)
        do { group(r, TbTag<true>{}); r += 3; } while (r < r_begin + TRIMMED && r < r_end);
    }
    if (marks) marks->steady = wall_clock64();
    for (; r < r_end; r += 3) group(r, TbTag<false>{});
}

// Does strip tx read a wall column?  The first and the last strip do; with the older placement (shift = HW) so does the
// last but one when the last strip holds at most HW columns of the mesh: the wall column then lies in its halo, and the
// sweeps it recomputes there need b (226 columns, T = 8: strip 1 reads columns 104...231).  Never so with shift = 0.
template <int T> __device__ __forceinline__ bool tb_wall_strip(int tx, int ntx, int shift, int nx)
{
    constexpr int HW = (T + 1) & ~1;
    return tx == 0 || tx == ntx - 1 || tx * (TB_COLS - 2 * HW) - shift + TB_COLS >= nx;
}

// grid: persistent workgroups of 4 waves.  Wave tiles (strip tx, chunk ty) are numbered
// strip-major (wt = tx*gy + ty) and dealt 4 per workgroup, so the 4 waves of a workgroup
// normally hold 4 vertically adjacent chunks of one strip (shared halo rows stay in L1/L2)
// and no wave idles because the strip count is not a multiple of 4.  `gx` = number of
// workgroup tiles = ceil(ntx*gy / 4); gy = nimg * cpi chunks.  nx must be even.
// Image k of a stack: mesh rows [dom_lo + k*img_stride, ... + ny), owned rows
// [own_lo + k*img_stride, ... + own_h).  Batch: dom_lo = own_lo = 0, own_h = img_stride = ny.
// Row slab (one image): dom_lo = -(first array row's global index), ny = global height,
// own_lo = halo depth, own_h = rows owned by this rank.
// (measurement switch: -DTB_ROWS_AUX=16 builds the dealt path of this kernel with device-coherent rows, to be timed against
// the plain build in one process -- tools/build_variant.sh; never set by the Makefile)
#ifndef TB_ROWS_AUX
#define TB_ROWS_AUX 0
#endif
// (the body of the kernel, shared with its pre-scaled form k_sweep_matfree_tb_pre below: `lut` is the table in LDS, loaded)
template <int T, bool FMA, bool GUARD, bool PRE = false>
__device__ __forceinline__ void tb_tiles(const double *lut, const uint16_t *__restrict__ code, const double *__restrict__ x,
                                         double *__restrict__ xnew, int nx, int ny, int img_stride, int dom_lo, int own_lo,
                                         int own_h, int cpi, const uint8_t *__restrict__ active, int LY, int ntx, int nbt, int gy,
                                         int flip, int xmajor, int allb, int shift, double omw,
                                         unsigned long long *__restrict__ stamps, const int4 *__restrict__ dealt)
{
    static_assert(T >= 1 && T <= 8, "unsupported T");
    const int lane = threadIdx.x & 63;
    // readfirstlane makes the wave index (and everything derived from it: strip, chunk, row
    // classes, loop bounds) provably wave-uniform, i.e. SGPR/SALU work; left as a VGPR it
    // costs ~80 VGPRs of per-lane copies of scalars
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned total = (unsigned)nbt;              // workgroup tiles
    const unsigned wtiles = (unsigned)ntx * (unsigned)gy;
    const unsigned per = (total + 7u) / 8u;
    const unsigned xcd = blockIdx.x & 7u;
    const unsigned nper = gridDim.x >> 3;

    // diagnostics only (tools/tb_stamps.py): wall-clock start / end of every wave tile; the buffer is
    // written by lane 0 after the tile and read by nobody on the device
    const unsigned long long t_begin = stamps ? wall_clock64() : 0ull;
    if (dealt) {
        // Dealt tiles (one tile per wave; plan_streaming / deal_ranked_tiles in api_sweep.hip): wave `wave` of workgroup
        // blockIdx.x runs the chunk the host wrote at dealt[4 * blockIdx.x + wave] = (strip | image << 16, first row, rows, stamp index) --
        // chunk heights then follow the order in which a SIMD serves its waves.  rows = 0: nothing for this wave.
        const int4 d = dealt[(size_t)blockIdx.x * 4u + (unsigned)wave];
        if (d.z <= 0) return;
        // the deal rests on an observation -- workgroup (blockIdx >> 3) / (CUs per XCD) of an XCD lands in wave slot 0, 1, 2 of its
        // SIMDs -- and watches it: a wave that finds itself in another slot than its tile was cut for counts itself in the word
        // behind the table; the host reads the count after the first launches of a plan and goes back to equal chunks if the
        // chip is not dispatching that way (another process on the GPU).  d.w = stamp index | slot << 30.
        if (lane == 0 && __builtin_amdgcn_s_getreg(0x1804) != ((unsigned)d.w >> 30))
            atomicAdd(reinterpret_cast<unsigned *>(const_cast<int4 *>(dealt) + (size_t)gridDim.x * 4u), 1u);
        const int tx = d.x & 0xFFFF, img = d.x >> 16;      // image of a stack
        if (active && !active[img]) return;
        const int row_lo = dom_lo + img * img_stride, own_hi = own_lo + img * img_stride + own_h;
        if (allb || tb_wall_strip<T>(tx, ntx, shift, nx))
            tb_strip<T, GUARD, true, FMA, TB_ROWS_AUX, true, PRE>(lut, code, x, xnew, nx, ny, row_lo, own_hi, tx, ntx, shift, d.y, d.z, lane, omw);
        else
            tb_strip<T, GUARD, false, FMA, TB_ROWS_AUX, true, PRE>(lut, code, x, xnew, nx, ny, row_lo, own_hi, tx, ntx, shift, d.y, d.z, lane, omw);
        if (stamps && lane == 0) {
            const unsigned long long where = (unsigned long long)(__builtin_amdgcn_s_getreg(0xF804) & 0xFFFFu) |
                                             ((unsigned long long)(__builtin_amdgcn_s_getreg(0xF814) & 0xFu) << 16);
            const size_t si = (size_t)(d.w & 0x3FFFFFFF);
            stamps[2 * si] = t_begin;
            stamps[2 * si + 1] = ((wall_clock64() - t_begin) & 0xFFFFFFFFull) | (where << 32);
        }
        return;
    }
    for (unsigned kk = blockIdx.x >> 3; kk < per; kk += nper) {
        const unsigned bt = xcd * per + (flip ? per - 1u - kk : kk);
        if (bt >= total) continue;
        const unsigned wt = bt * 4u + (unsigned)wave;
        if (wt >= wtiles) continue;                    // wave-uniform
        // strip-major: 4 waves = 4 stacked chunks of one strip; x-major: 4 neighbouring strips
        const int tx = xmajor ? (int)(wt % (unsigned)ntx) : (int)(wt / (unsigned)gy);
        const int bty = xmajor ? (int)(wt / (unsigned)ntx) : (int)(wt % (unsigned)gy);
        const int img = bty / cpi;                     // cpi chunks per image, gy = nimg * cpi
        if (active && !active[img]) continue;          // frozen image of a batch
        const int row_lo = dom_lo + img * img_stride;
        const int own0 = own_lo + img * img_stride;
        const int ry0 = own0 + (bty - img * cpi) * LY;

        // b is read only where it can be non-zero: strips holding a wall column, or everywhere for a
        // harvested dictionary whose right-hand side is not confined to the walls
        if (allb || tb_wall_strip<T>(tx, ntx, shift, nx))
            tb_strip<T, GUARD, true, FMA, 0, false, PRE>(lut, code, x, xnew, nx, ny, row_lo, own0 + own_h, tx, ntx, shift, ry0, LY, lane, omw);
        else
            tb_strip<T, GUARD, false, FMA, 0, false, PRE>(lut, code, x, xnew, nx, ny, row_lo, own0 + own_h, tx, ntx, shift, ry0, LY, lane, omw);
        if (stamps && lane == 0) {
            // end stamp: low 32 bits = duration in 10-ns ticks, bits 32...47 = HW_ID (wave slot, SIMD, CU, SE), 48...51 = XCC
            const unsigned long long where = (unsigned long long)(__builtin_amdgcn_s_getreg(0xF804) & 0xFFFFu) |
                                             ((unsigned long long)(__builtin_amdgcn_s_getreg(0xF814) & 0xFu) << 16);
            stamps[2 * (size_t)wt] = t_begin;
            stamps[2 * (size_t)wt + 1] = ((wall_clock64() - t_begin) & 0xFFFFFFFFull) | (where << 32);
        }
    }
}

template <int T, bool FMA, bool GUARD>
__global__ __launch_bounds__(256, (T >= 6 ? 3 : 1)) void k_sweep_matfree_tb(const double *__restrict__ lut_g,
                                                          const uint16_t *__restrict__ code,
                                                          const double *__restrict__ x,
                                                          double *__restrict__ xnew, int nx, int ny,
                                                          int img_stride, int dom_lo, int own_lo,
                                                          int own_h, int cpi,
                                                          const uint8_t *__restrict__ active,
                                                          int LY, int ntx, int nbt, int gy, int flip,
                                                          int xmajor, int allb, int nrows, int shift,
                                                          double omw, unsigned long long *__restrict__ stamps,
                                                          const int4 *__restrict__ dealt)
{
    __shared__ double lut[LUT_DOUBLES];
    load_lut(lut, lut_g, nrows);
    tb_tiles<T, FMA, GUARD>(lut, code, x, xnew, nx, ny, img_stride, dom_lo, own_lo, own_h, cpi, active, LY, ntx, nbt, gy, flip, xmajor,
                            allb, shift, omw, stamps, dealt);
}

// The pre-scaled form (kernels_sweep.hpp, pre_cell): the same tiles, dealt or not, over the pre-scaled table lut_g; `allb`
// here also covers a table whose b' is not +0.0 on every row away from the walls.  Same arguments as k_sweep_matfree_tb.
template <int T>
__global__ __launch_bounds__(256, (T >= 6 ? 3 : 1)) void k_sweep_matfree_tb_pre(const double *__restrict__ lut_g,
                                                          const uint16_t *__restrict__ code,
                                                          const double *__restrict__ x,
                                                          double *__restrict__ xnew, int nx, int ny,
                                                          int img_stride, int dom_lo, int own_lo,
                                                          int own_h, int cpi,
                                                          const uint8_t *__restrict__ active,
                                                          int LY, int ntx, int nbt, int gy, int flip,
                                                          int xmajor, int allb, int nrows, int shift,
                                                          double omw, unsigned long long *__restrict__ stamps,
                                                          const int4 *__restrict__ dealt)
{
    __shared__ double lut[LUT_DOUBLES];
    load_lut(lut, lut_g, nrows);
    tb_tiles<T, true, false, true>(lut, code, x, xnew, nx, ny, img_stride, dom_lo, own_lo, own_h, cpi, active, LY, ntx, nbt, gy, flip,
                                   xmajor, allb, shift, omw, stamps, dealt);
}

// ---------------------------------------------------------------------------------------------------------------
// Flags between the tiles of ONE launch: shared by the chained streaming kernel below and the resident workgroup tiles
// (kernels_wgtile.hpp, where the protocol and its history are described).  A flag holds the number of passes its tile has
// published; a tile's data is stored device-coherently (aux bit sc1), acknowledged, and only then counted.
constexpr unsigned long long WGR_TIMEOUT = 200000000ull;       // 2 s of the 100 MHz wall clock
constexpr int WGR_FLAG_STRIDE = 64;                            // unsigneds between two tiles' flags: one 256-byte block each, so that
                                                               // ~2 000 polling lanes do not queue on a handful of cache lines
constexpr int WGR_SC1 = 16;                                    // aux bit 4 of the raw buffer intrinsics on gfx94x/gfx950

// One lane waits until *flag has reached `want` (signed difference: the count may wrap).  Bounded: a lane that has polled for
// WGR_TIMEOUT, or that sees *abort_flag set, raises *abort_flag and returns true -- so does, within 32 polls, every lane
// waiting anywhere; the caller then leaves the kernel (the host redoes the interval, resident_check in api_sweep.hip).
__device__ __forceinline__ bool wgr_wait_flag(const unsigned *flag, unsigned want, unsigned *abort_flag)
{
    const unsigned long long t0 = wall_clock64();
    unsigned polls = 0;
    while ((int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
        __builtin_amdgcn_s_sleep(1);
        if ((++polls & 31u) == 0u &&
            (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || wall_clock64() - t0 > WGR_TIMEOUT)) {
            __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
    }
    return false;
}

// Chained passes: `npass` passes of the dealt tiles in ONE launch.  The grid is exactly the co-resident one (three workgroups
// per CU, one tile per wave: deal_ranked_tiles), so every tile is on the chip for the whole launch and a launch boundary --
// a chip-wide barrier that leaves every SIMD on two waves, then one, then none until the slowest tile of the chip has ended --
// is replaced by what the next pass really needs: the tiles whose rows a tile's window reads, and those that still read the
// rows it is about to overwrite (nbrs: up to TB_CHAIN_NB table slots per wave, each + 1, 0 = none; tb_chain.hpp computes them on the
// host from the same geometry as tb_strip).  Pass p reads xa and writes xb when p is even, the other way round when odd.
//   before pass p > 0   lanes 0...TB_CHAIN_NB-1 poll one neighbour's flag each until it reads base + p;
//   after pass p        (not the last: the end of the launch publishes that) the wave waits for its stores' acknowledgement
//                       and lane 0 stores base + p + 1 to its own flag.
// Waves are independent: no workgroup barrier after the dictionary load.  The rows travel device-coherently (tb_strip's XAUX =
// sc1) from the first pass on, the codes -- constant -- through plain loads.  Same tiles, same arithmetic, same bits as
// npass launches of k_sweep_matfree_tb on the same table.  `miss`: the dealt-slot miss counter (see k_sweep_matfree_tb).
// stamps (tools/tb_stamps.py --chain): word 0 of the buffer = the first pass to stamp (set by the host, so that three passes
// DEEP in a chain can be looked at), word 1 unused; then TB_CHAIN_STAMPS words per tile -- entry, where it ran, and for the
// passes first ... first + 2 {neighbours seen, first row consumed, steady-state loop entered, swept = last store issued,
// stores acknowledged, flag published}.
constexpr int TB_CHAIN_STAMPS = 20, TB_CHAIN_STAMP_HEAD = 2;
constexpr int TB_CHAIN_NB = 16;
template <int T, bool FMA, bool GUARD>
__global__ __launch_bounds__(256, (T >= 6 ? 3 : 1)) void k_sweep_matfree_tb_chain(const double *__restrict__ lut_g,
                                                          const uint16_t *__restrict__ code, double *xa, double *xb,
                                                          int nx, int ny, int img_stride, int dom_lo, int own_lo,
                                                          int own_h, int ntx, int allb, int nrows, int shift, double omw,
                                                          const int4 *__restrict__ dealt, const unsigned *__restrict__ nbrs,
                                                          unsigned *miss, int npass, unsigned *flags, unsigned base,
                                                          unsigned *abort_flag, unsigned long long *stamps)
{
    static_assert(T >= 1 && T <= 8, "unsupported T");
    __shared__ double lut[LUT_DOUBLES];
    load_lut(lut, lut_g, nrows);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t slot = (size_t)blockIdx.x * 4u + (unsigned)wave;
    const int4 d = dealt[slot];
    if (d.z <= 0) return;                                          // a wave without a tile: in nobody's list
    if (lane == 0 && __builtin_amdgcn_s_getreg(0x1804) != ((unsigned)d.w >> 30)) atomicAdd(miss, 1u);
    const int tx = d.x & 0xFFFF, img = d.x >> 16;
    const int row_lo = dom_lo + img * img_stride, own_hi = own_lo + img * img_stride + own_h;
    unsigned long long *st = stamps ? stamps + TB_CHAIN_STAMP_HEAD + (size_t)(d.w & 0x3FFFFFFF) * TB_CHAIN_STAMPS : nullptr;     // (wave-uniform; lane 0 writes)
    const int st_first = stamps ? (int)stamps[0] : 0;
    if (st && lane == 0) {
        st[0] = wall_clock64();
        st[1] = (unsigned long long)(__builtin_amdgcn_s_getreg(0xF804) & 0xFFFFu) | ((unsigned long long)(__builtin_amdgcn_s_getreg(0xF814) & 0xFu) << 16);
    }
    auto passes = [&](auto wall_tag) __attribute__((always_inline)) {
        constexpr bool WALL = decltype(wall_tag)::value;
#pragma unroll 1
        for (int p = 0; p < npass; ++p) {
            if (p > 0) {
                // (the list is read again in every pass rather than kept -- a register the row loop does not have --, through a
                // descriptor of this wave's TB_CHAIN_NB entries: no per-lane address to keep either; lanes beyond it read 0.
                // Asking for it one round trip earlier, in the shadow of the stores' acknowledgement below, was measured and
                // bought nothing: DESIGN.md section 4, profiles/r07_tb_chain_boundary.log)
                const unsigned nb = __builtin_amdgcn_raw_buffer_load_b32(tb_rsrc(nbrs + slot * TB_CHAIN_NB, TB_CHAIN_NB * 4u), lane * 4, 0, 0);
                bool bad = false;
                if (nb != 0u) bad = wgr_wait_flag(flags + (size_t)(nb - 1u) * WGR_FLAG_STRIDE, base + (unsigned)p, abort_flag);
                if (__builtin_amdgcn_ballot_w64(bad) != 0ull) return;       // wave-uniform: this wave gives up
                // the rows are asked for after the flags were seen: the polls' values have arrived (the loop's exit depends on
                // them) and the compiler moves no memory access across this line
                asm volatile("" ::: "memory");
            }
            unsigned long long *sp = (st && p >= st_first && p < st_first + 3) ? st + 2 + 6 * (p - st_first) : nullptr;   // (wave-uniform)
            if (sp && lane == 0) sp[0] = wall_clock64();
            const double *src = (p & 1) ? xb : xa;
            double *dst = (p & 1) ? xa : xb;
            // (the two clocks are read whether or not anybody stamps: a wave-uniform test around them would cut the ramp's
            // basic block in two, and the compiler sinks row requests across such a cut -- two scalar clock reads per pass)
            TbMarks mk = {0ull, 0ull};
            // (To the compiler: nothing is in flight here -- the wait behind the previous pass is inline assembly, which its
            // count of the operations in flight does not read, and what it believes pending from there would reach the
            // steady-state loop's waits along an edge of the emitted control flow that is never taken.  At run time the counter
            // is at zero already: the polls' values have arrived, and they return behind everything older.)
            __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0) alone
            tb_strip<T, GUARD, WALL, FMA, WGR_SC1>(lut, code, src, dst, nx, ny, row_lo, own_hi, tx, ntx, shift, d.y, d.z, lane, omw, &mk);
            if (sp && lane == 0) { sp[1] = mk.first_row; sp[2] = mk.steady; sp[3] = wall_clock64(); }
            if (p + 1 < npass) {
                // the stores acknowledged (written through to the coherence point), then the flag: spelled out, see wgres_body
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (sp && lane == 0) sp[4] = wall_clock64();
                if (lane == 0)
                    __hip_atomic_store(flags + slot * WGR_FLAG_STRIDE, base + (unsigned)p + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (sp && lane == 0) sp[5] = wall_clock64();
            }
        }
    };
    if (allb || tb_wall_strip<T>(tx, ntx, shift, nx)) passes(TbTag<true>{});
    else passes(TbTag<false>{});
}

}  // namespace deff
