// kernels_cg_fold.hpp -- the conjugate-gradient iteration in two launches instead of four (tuning key "cg_fold", api_cg.hip,
// DESIGN.md section 9 "Fold"): the streaming launches of kernels_cg.hpp (table form) and kernels_cg_planes.hpp (plane form)
// with the per-image reductions k_cg_alpha / k_cg_beta folded in.  FP64, gfx950 wave64.
//
//   k_cgf_dir     k_cg_dir,     then alpha = rho / p'.Ap' by the image's last workgroup to arrive
//   k_cgf_dir2    k_cgf_dir with the loads of a row ahead in flight ("cg_fold" 2)
//   k_cgf_update  k_cg_update,  then k_cg_beta's step by the image's last workgroup to arrive
//   k_cgpf_dir / k_cgpf_update  the same around k_cgp_dir / k_cgp_update
//
// The tail.  Every image has two sets of counters (cg_tick: one for the direction launch, one for the update launch), zeroed
// by the host at the start of every call.  A wave that has stored its item's partial(s) adds 1 to a counter of its image; the
// wave whose add completes the image is the image's last and marks the image in LDS.  Behind a workgroup barrier the whole
// workgroup runs k_cg_alpha's / k_cg_beta's sum and step for every marked image (up to four: one per wave) and puts the counter
// back to 0.  The counting has two levels: adds to one address are served one after the other, about 10 ns each, so one
// counter per image costs 4 096 items 40 us (measured: DESIGN.md).  An image's items are counted in shards of CGF_SHARD
// consecutive items, every counter on 256 bytes of its own; the wave that completes a shard resets it and adds 1 to the
// image's counter, and the wave whose add there returns shards - 1 is the image's last.
// Nothing waits for another workgroup, so nothing can hang.  No wave returns before that barrier: waves beyond the last item
// and waves of a frozen image (done != 0) go there without a tick.
//
// Visibility between workgroups (per-XCD L2s are not coherent, a compute unit's L1 is never refreshed by another's stores):
// the partials are stored write-through (8-byte relaxed agent-scope atomic stores, vector stores of lane 63), the storing wave
// waits for them (s_waitcnt vmcnt(0)) and then adds to the counter (relaxed, agent scope); the lane whose add came last runs
// one agent-scope acquire fence + s_waitcnt vmcnt(0) -- the reducer reads the same addresses every iteration, its L1 is warm
// with the last iteration's partials --, then the barrier, then plain loads.  One acquire per image and launch, no release
// anywhere: an agent-scope release in the streaming workgroups would write back the L2 lines their own p', x, r stores have
// just dirtied.
//
// Bits: a folded kernel calls the row walk of the four-launch kernel it folds (cg_dir_rows, cg_update_rows of kernels_cg.hpp;
// cgp_dir_rows, cgp_update_rows of kernels_cg_planes.hpp) on the same work items (cg_item) and partial slots, and its tail
// the same sum and scalar step (cg_image_sum, cg_alpha_step, cg_beta_step): every result is the four-launch form's.
// k_cgf_dir2 alone has a row walk of its own -- another load discipline around the same cg_apply, in the same order.
// The per-image scalars are written by a tail while other images' items still read theirs: `sc` is neither const nor
// __restrict__ here.  An image's items have all read beta / restart / alpha before they tick, so its tail may overwrite them.
#pragma once
#include "kernels_cg.hpp"
#include "kernels_cg_planes.hpp"

namespace deff {

constexpr unsigned CGF_SHARD = 64;              // items per first-level counter
constexpr unsigned CGF_PAD = 64;                // unsigneds from one counter to the next

// counters of one launch kind: per image its own counter, then one per shard
__host__ __device__ inline unsigned cgf_shards(unsigned per_img) { return (per_img + CGF_SHARD - 1) / CGF_SHARD; }
__host__ __device__ inline size_t cgf_ticks(unsigned per_img, size_t nimg) { return nimg * (1 + cgf_shards(per_img)) * CGF_PAD; }
__device__ __forceinline__ unsigned *cgf_tick_of(unsigned *tick, unsigned per_img, int img)
{
    return tick + (size_t)img * (1 + cgf_shards(per_img)) * CGF_PAD;
}

constexpr int CGF_LDS = 8;                      // doubles of LDS of the tail: 4 wave sums, 4 ints (the image wave w finished, or -1)

__device__ __forceinline__ void cgf_store(double *p, double v)           // write-through
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// A wave of a folded launch: its item, and whether it has work (`run`: the item exists and its image is not frozen).  ws / mark:
// the tail's LDS, CGF_LDS doubles.
struct CgfWave {
    int lane, wave;
    CgItem it;
    bool run;
    double *ws;
    int *mark;
};

// The start of every wave of a folded launch (a table-form kernel loads its table first).  No wave returns here.
__device__ __forceinline__ CgfWave cgf_begin(const CgGeom &g, const CgScal *sc, double *lds)
{
    CgfWave w;
    w.ws = lds;
    w.mark = reinterpret_cast<int *>(lds + 4);
    w.lane = threadIdx.x & 63;
    w.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    w.it.img = 0;
    w.it.idx = 0;
    w.run = cg_item(g, w.wave, w.lane, w.it);
    if (w.run) w.run = sc[w.it.img].done == 0;                    // frozen image: no writes, no tick
    return w;
}

// The end of every wave of a folded launch: a wave that ran has stored the partials of its item.  Returns behind the
// workgroup barrier; mark[v] is then the image wave v was the last of, or -1.
__device__ __forceinline__ void cgf_arrive(const CgfWave &w, unsigned per_img, unsigned *tick)
{
    if (w.lane == 63) {
        int m = -1;
        if (w.run) {
            const int img = w.it.img;
            unsigned *ti = cgf_tick_of(tick, per_img, img);
            const unsigned sh = (w.it.idx - (unsigned)img * per_img) / CGF_SHARD;
            const unsigned full = min(CGF_SHARD, per_img - sh * CGF_SHARD);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the partials have left
            unsigned *ts = ti + (size_t)(1 + sh) * CGF_PAD;
            if (__hip_atomic_fetch_add(ts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == full - 1u) {
                // every wave of the shard has waited for its stores before its add: the shard is in memory
                __hip_atomic_store(ts, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__hip_atomic_fetch_add(ti, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == cgf_shards(per_img) - 1u) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    m = img;
                }
            }
        }
        w.mark[w.wave] = m;
    }
    __syncthreads();
}

// k_cg_alpha's step for every image this workgroup was the last of (done == 0: a frozen image does not tick)
__device__ __forceinline__ void cgf_tail_alpha(const double *part, unsigned per_img, CgScal *sc, unsigned *tick, const CgfWave &w)
{
    for (int k = 0; k < 4; ++k) {
        const int img = w.mark[k];
        if (img < 0) continue;
        const double pap = cg_image_sum(part + (size_t)img * per_img, per_img, 1, 0, w.ws);
        if (threadIdx.x == 0) {
            cg_alpha_step(sc[img], pap);
            __hip_atomic_store(cgf_tick_of(tick, per_img, img), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// k_cg_beta's step likewise
__device__ __forceinline__ void cgf_tail_beta(const double *part_rz, const double *part_rr, unsigned per_img, CgScal *sc,
                                              double tol2, long long max_iter, unsigned *tick, const CgfWave &w)
{
    for (int k = 0; k < 4; ++k) {
        const int img = w.mark[k];
        if (img < 0) continue;
        const double rz = cg_image_sum(part_rz + (size_t)img * per_img, per_img, 1, 0, w.ws);
        const double rr = cg_image_sum(part_rr + (size_t)img * per_img, per_img, 1, 0, w.ws);
        if (threadIdx.x == 0) {
            cg_beta_step(sc[img], rz, rr, tol2, max_iter);
            __hip_atomic_store(cgf_tick_of(tick, per_img, img), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- table form --------------------------------------------------------------------------------------------------------

// Launch A: k_cg_dir's item (cg_dir_rows), then the tail.
__global__ __launch_bounds__(256) void k_cgf_dir(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                 const double *__restrict__ r, const double *__restrict__ p_in,
                                                 double *__restrict__ p_out, CgScal *sc, CgGeom g, double *partial, unsigned *tick)
{
    __shared__ double tab[CG_DOUBLES + CGF_LDS];
    cg_load_tab(tab, tab_g, nrows);
    const CgfWave w = cgf_begin(g, sc, tab + CG_DOUBLES);
    if (w.run) {
        const CgItem &it = w.it;
        const double s = cg_dir_rows(tab, code, r, p_in, p_out, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                                     cg_halo_col(g.nx, it.col, w.lane), sc[it.img].restart != 0, sc[it.img].beta, false, false);
        if (w.lane == 63) cgf_store(partial + it.idx, s);
    }
    cgf_arrive(w, g.per_img, tick);
    cgf_tail_alpha(partial, g.per_img, sc, tick, w);
}

// what p' of a lane's two cells / of its halo cell is made of
struct CgfRaw2 {
    double2 r, p;
    unsigned cw;
};
struct CgfRaw1 {
    double r, p;
    unsigned cw;
};

// Launch A with the loads of a row ahead in flight ("cg_fold" 2): k_cgp_dir's discipline on the table form.  In front of row
// l's arithmetic the loads of what p' of row l + 2 is made of (r, p, the codes) and of row l + 1's halo cell are issued into
// the register set that row l does not read; the two sets take turns in a loop unrolled by two, the item's last row asks for
// nothing.  No load sits behind a branch: every lane loads from a clamped address (a lane beyond the row's end the row's
// first cells, a row outside the image the nearest one inside, p even on a restart) and what may not count is zeroed
// afterwards.  Addresses are a scalar row base + the lane's 32-bit byte offset.  The arithmetic and its order are k_cg_dir's.
__global__ __launch_bounds__(256) void k_cgf_dir2(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                  const double *__restrict__ r, const double *__restrict__ p_in,
                                                  double *__restrict__ p_out, CgScal *sc, CgGeom g, double *partial, unsigned *tick)
{
    __shared__ double tab[CG_DOUBLES + CGF_LDS];
    cg_load_tab(tab, tab_g, nrows);
    const CgfWave w = cgf_begin(g, sc, tab + CG_DOUBLES);
    if (w.run) {
        const CgItem &it = w.it;
        const int lane = w.lane;
        const bool restart = sc[it.img].restart != 0;
        // (what is the same in every lane is kept in scalar registers: the vector registers go to the rows in flight)
        const double bv = sc[it.img].beta;
        const double beta = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(bv)),
                                             __builtin_amdgcn_readfirstlane(__double2loint(bv)));
        const int l0 = __builtin_amdgcn_readfirstlane(it.l0), l1 = __builtin_amdgcn_readfirstlane(it.l1);
        const bool v = it.col < g.nx;
        const int jh = cg_halo_col(g.nx, it.col, lane);
        const unsigned cb = v ? (unsigned)it.col * 8u : 0u, hb = (unsigned)max(jh, 0) * 8u;
        auto row_of = [&](const void *a, int l, int cell) {
            return cgp_uniform(reinterpret_cast<const double *>(
                reinterpret_cast<const char *>(a) + (it.base + (size_t)min(max(l, 0), g.ny - 1) * g.nx) * (size_t)cell));
        };
        auto inside = [&](int l) { return v && l >= 0 && l < g.ny; };
        // A lane offset is handed over where it is used, as the 32 bits it is: widened to 64 bits once in front of the loop it
        // would cost a register pair per array and one more per address, and the fifth wave per SIMD with them.
        auto here = [](unsigned o) { asm volatile("" : "+v"(o)); return o; };
        auto raw2 = [&](int l) -> CgfRaw2 {
            CgfRaw2 o;
            const unsigned c8 = here(cb);
            o.r = cgp_gld2(row_of(r, l, 8), c8);
            o.p = cgp_gld2(row_of(p_in, l, 8), c8);
            o.cw = *(const unsigned __attribute__((address_space(1))) *)(row_of(code, l, 2) + (c8 >> 2));
            return o;
        };
        auto raw1 = [&](int l) -> CgfRaw1 {
            CgfRaw1 o;
            const unsigned h8 = here(hb);
            o.r = cgp_gld1(row_of(r, l, 8), h8);
            o.p = cgp_gld1(row_of(p_in, l, 8), h8);
            // its code: the aligned pair of codes that holds it (the pitch is even), the half picked where it is used
            o.cw = *(const unsigned __attribute__((address_space(1))) *)(row_of(code, l, 2) + ((h8 >> 2) & ~3u));
            return o;
        };
        auto pn2 = [&](const CgfRaw2 &o, int l) -> double2 {      // p' of the lane's two cells of row l (0 outside)
            const double2 z = make_double2(o.r.x * cg_v<CG_INV>(tab, o.cw & 0xFFFFu), o.r.y * cg_v<CG_INV>(tab, o.cw >> 16));
            const double2 t = restart ? z : make_double2(z.x + beta * o.p.x, z.y + beta * o.p.y);
            return inside(l) ? t : make_double2(0.0, 0.0);
        };
        auto pn1 = [&](const CgfRaw1 &o) -> double {
            const double z = o.r * cg_v<CG_INV>(tab, (o.cw >> ((here(hb) & 8u) << 1)) & 0xFFFFu);
            const double t = restart ? z : z + beta * o.p;
            return jh >= 0 ? t : 0.0;
        };
        const CgfRaw2 r0 = raw2(l0 - 1), r1 = raw2(l0);
        CgfRaw2 da = raw2(l0 + 1), db = da;                       // row l + 1, row l + 2
        CgfRaw1 ha = raw1(l0), hb1 = ha;                          // halo cell of row l, of row l + 1
        double2 up = pn2(r0, l0 - 1), cur = pn2(r1, l0);
        unsigned cw = v ? r1.cw : 0u;
        double acc = 0.0;
        // row l: `d` holds what row l + 1 is made of and `h` row l's halo cell; `dn` / `hn` take the requests of the turn after
        auto step = [&](auto more_c, int l, const CgfRaw2 &d, const CgfRaw1 &h1, CgfRaw2 &dn2, CgfRaw1 &hn) {
            constexpr bool MORE = decltype(more_c)::value;
            if constexpr (MORE) {
                dn2 = raw2(l + 2);
                hn = raw1(l + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            const double2 dn = pn2(d, l + 1);
            const double h = pn1(h1);
            const unsigned cw_dn = v ? d.cw : 0u;
            const double2 ap = cg_apply(tab, cw & 0xFFFFu, cw >> 16, cur, up, dn, h);
            acc += cur.x * ap.x + cur.y * ap.y;
            if (v) cgp_gst2(row_of(p_out, l, 8), here(cb), cur);
            up = cur;
            cur = dn;
            cw = cw_dn;
        };
        const std::true_type more;
        const std::false_type last;
        int l = l0;
#pragma unroll 1
        for (; l + 2 < l1; l += 2) {
            step(more, l, da, ha, db, hb1);
            step(more, l + 1, db, hb1, da, ha);
        }
        if (l + 1 < l1) {
            step(more, l, da, ha, db, hb1);
            step(last, l + 1, db, hb1, da, ha);
        } else step(last, l, da, ha, db, hb1);
        const double s = wave_sum_to_lane63(acc);
        if (lane == 63) cgf_store(partial + it.idx, s);
    }
    cgf_arrive(w, g.per_img, tick);
    cgf_tail_alpha(partial, g.per_img, sc, tick, w);
}

// Launch B: k_cg_update's item (cg_update_rows), then the tail.
__global__ __launch_bounds__(256) void k_cgf_update(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                    const double *__restrict__ p, double *__restrict__ x, double *__restrict__ r,
                                                    CgScal *sc, CgGeom g, double *partial_rz, double *partial_rr, double tol2,
                                                    long long max_iter, unsigned *tick)
{
    __shared__ double tab[CG_DOUBLES + CGF_LDS];
    cg_load_tab(tab, tab_g, nrows);
    const CgfWave w = cgf_begin(g, sc, tab + CG_DOUBLES);
    if (w.run) {
        const CgItem &it = w.it;
        double s1, s2;
        cg_update_rows(tab, code, p, x, r, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                       cg_halo_col(g.nx, it.col, w.lane), sc[it.img].alpha, s1, s2);
        if (w.lane == 63) { cgf_store(partial_rz + it.idx, s1); cgf_store(partial_rr + it.idx, s2); }
    }
    cgf_arrive(w, g.per_img, tick);
    cgf_tail_beta(partial_rz, partial_rr, g.per_img, sc, tol2, max_iter, tick, w);
}

// ---- plane form --------------------------------------------------------------------------------------------------------

// Launch A: k_cgp_dir's item (cgp_dir_rows, its rolling window of loads included), then the tail.
__global__ __launch_bounds__(256) void k_cgpf_dir(CgpPlanes A, const double *__restrict__ inv, const double *__restrict__ r,
                                                  const double *__restrict__ p_in, double *__restrict__ p_out,
                                                  double *__restrict__ q_out, CgScal *sc, CgGeom g, double *partial, unsigned *tick)
{
    __shared__ double lds[CGF_LDS];
    const CgfWave w = cgf_begin(g, sc, lds);
    if (w.run) {
        const CgItem &it = w.it;
        const double s = cgp_dir_rows(A, inv, r, p_in, p_out, q_out, cg_win(g, it), g.nx, it.col, it.l0, it.l1,
                                      cg_halo_col(g.nx, it.col, w.lane), sc[it.img].restart != 0, sc[it.img].beta);
        if (w.lane == 63) cgf_store(partial + it.idx, s);
    }
    cgf_arrive(w, g.per_img, tick);
    cgf_tail_alpha(partial, g.per_img, sc, tick, w);
}

// Launch B: k_cgp_update's item (cgp_update_rows), then the tail.
__global__ __launch_bounds__(256) void k_cgpf_update(const double *__restrict__ inv, const double *__restrict__ p,
                                                     const double *__restrict__ qv, double *x, double *r, CgScal *sc, CgGeom g,
                                                     double *partial_rz, double *partial_rr, double tol2, long long max_iter,
                                                     unsigned *tick)
{
    __shared__ double lds[CGF_LDS];
    const CgfWave w = cgf_begin(g, sc, lds);
    if (w.run) {
        const CgItem &it = w.it;
        double s1, s2;
        cgp_update_rows(inv, p, qv, x, r, cg_win(g, it), g.nx, it.col, it.l0, it.l1, sc[it.img].alpha, s1, s2);
        if (w.lane == 63) { cgf_store(partial_rz + it.idx, s1); cgf_store(partial_rr + it.idx, s2); }
    }
    cgf_arrive(w, g.per_img, tick);
    cgf_tail_beta(partial_rz, partial_rr, g.per_img, sc, tol2, max_iter, tick, w);
}

}  // namespace deff
