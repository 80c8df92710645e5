// api_sweep.hip -- everything that plans or launches a sweep: the planner of a temporally blocked pass (which form, which
// tile, which grid), the dealt tiles of the streaming form, the resident-launch protocol, the launchers and deff_sweeps().
// The workgroup-tile kernels are instantiated in tiles_*.hip (tile_kernels.hpp); the streaming and single-sweep kernels here.
// See ctx.hpp for the file map, DESIGN.md section 4 for the design.
#include "ctx.hpp"
#include "tile_kernels.hpp"
#include "tb_chain.hpp"
#include <map>
#include <mutex>

// ----------------------------------------------------------- sweeps -------

// Streaming form (kernels_tb.hpp), [tb_index(T)][2 fma + guard].  Only 2 cells per lane are instantiated: 4 per lane (twice the
// work per wave, 244 VGPRs, 2 waves per SIMD) measured 20 % slower at 4096^2 -- the kernel needs the wave-level parallelism more
// than it needs the smaller strip overlap.
template <int... T> static constexpr auto streaming_passes()
{
    return std::array{by_flags([](auto f, auto g) { return k_sweep_matfree_tb<T, decltype(f)::value, decltype(g)::value>; })...};
}
static constexpr auto STREAMING = streaming_passes<1, 2, 4, 6, 8>();
// ... and its chained form, [2 fma + guard]: dealt tiles exist for T = 8 only (plan_streaming)
static constexpr auto STREAMING_CHAIN = by_flags([](auto f, auto g) { return k_sweep_matfree_tb_chain<8, decltype(f)::value, decltype(g)::value>; });
static_assert(TB_CHAIN_NB == TB_CHAIN_MAXN && TB_CHAIN_COLS == TB_COLS && sizeof(TbChainTile) == sizeof(int4), "tb_chain.hpp and kernels_tb.hpp disagree");
// ... and its pre-scaled form (tuning "prescaled"), [tb_index(T)]: one launch per pass, never chained
static constexpr std::array STREAMING_PRE = {k_sweep_matfree_tb_pre<1>, k_sweep_matfree_tb_pre<2>, k_sweep_matfree_tb_pre<4>,
                                             k_sweep_matfree_tb_pre<6>, k_sweep_matfree_tb_pre<8>};
static int tb_index(int T) { return T == 1 ? 0 : T == 2 ? 1 : T == 4 ? 2 : T == 6 ? 3 : 4; }

// The first workgroup tile (tile_kernels.hpp) that pred accepts: 8-wave, tall, 12-wave tiles, each list in its order.
template <class Pred> static const TileKernel *find_tile(Pred pred)
{
    const TileKernel *hit = nullptr;
    auto first_in = [&](const auto &list) {
        for (const TileKernel &t : list)
            if (pred(t)) { hit = &t; return true; }
        return false;
    };
    (void)(first_in(TILES_8WAVE) || first_in(TILES_TALL) || first_in(TILES_12WAVE));
    return hit;
}

static int cu_count(const deff_ctx *c, int *cus)
{
    HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, c->device));
    return DEFF_OK;
}

// Workgroups of `kernel` (blocks of `threads`) resident at once on this device: asked for every candidate by every plan, so
// remembered per (device, kernel).
template <class Kernel> static int resident_blocks(const deff_ctx *c, Kernel kernel, int threads, int *resident)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, int> cache;
    const std::pair<int, const void *> key(c->device, reinterpret_cast<const void *>(kernel));
    {
        std::lock_guard<std::mutex> lock(mu);
        const auto it = cache.find(key);
        if (it != cache.end()) { *resident = it->second; return DEFF_OK; }
    }
    int per_cu = 0, cus = 0;
    TRY(cu_count(c, &cus));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0));
    *resident = per_cu * cus;
    std::lock_guard<std::mutex> lock(mu);
    cache[key] = *resident;
    return DEFF_OK;
}

// Resident launches of this process, chained per device: a resident kernel must have all its workgroups on the chip to
// make progress, so two of them (two contexts on one GPU: deff2d --devices 0,0, a thread pool) must never be dispatched
// side by side -- each waits for the previous one's end.  Finite kernels of other streams only delay a resident launch.
static std::mutex g_res_mu;
static hipEvent_t g_res_ev[64];
static bool g_res_has[64];
static int g_res_users[64];          // contexts alive per device: the chain's event goes with the last of them

void resident_chain_ctx_created(int device)
{
    if (device < 0 || device >= 64) return;
    std::lock_guard<std::mutex> lock(g_res_mu);
    ++g_res_users[device];
}

// (called by deff_destroy with the device current and the context's stream drained)
void resident_chain_ctx_destroyed(int device)
{
    if (device < 0 || device >= 64) return;
    std::lock_guard<std::mutex> lock(g_res_mu);
    if (--g_res_users[device] > 0 || !g_res_has[device]) return;
    (void)hipEventDestroy(g_res_ev[device]);     // nobody is left to wait on it; the next context of this device starts a new chain
    g_res_has[device] = false;
}

static hipError_t resident_chain_begin(const deff_ctx *c)
{
    const int d = c->device;
    if (d < 0 || d >= 64) return hipSuccess;
    if (!g_res_has[d]) {
        hipError_t e = hipEventCreateWithFlags(&g_res_ev[d], hipEventDisableTiming);
        if (e != hipSuccess) return e;
        g_res_has[d] = true;
        return hipSuccess;                                          // nothing to wait for yet
    }
    return hipStreamWaitEvent(c->stream, g_res_ev[d], 0);
}

static hipError_t resident_chain_end(const deff_ctx *c)
{
    const int d = c->device;
    if (d < 0 || d >= 64 || !g_res_has[d]) return hipSuccess;
    return hipEventRecord(g_res_ev[d], c->stream);
}

// One resident launch of the plan's tile kernel (all of them take this argument list)
static hipError_t launch_resident(deff_ctx *c, const SweepPlan &pl, double *xa, double *xb, int npass, unsigned base)
{
    unsigned long long *stamps = c->tb_stamps;
    unsigned xbytes = (unsigned)(c->n * sizeof(double));
    int stall_tile = c->tb_debug_stall - 1;
    if (stall_tile >= 0 && c->tb_debug_stall_skip > 0) { --c->tb_debug_stall_skip; stall_tile = -1; }   // tests: a LATER launch stalls
    const double *lut = c->lut;
    const uint16_t *code = c->code;
    int nx = c->nx, ny = c->mesh_ny, img_stride = c->ny, dom_lo = c->dom_lo, own_lo = pl.own_lo, own_h = pl.own_h;
    int cpi = pl.tcpi, ly = pl.LY, ntx = pl.ntx, gy = pl.tgy, xmajor = c->tb_xmajor;
    int allb = (c->lut_allb || c->nx != c->nxt) ? 1 : 0, nrows = c->lut_nrows, shift = pl.shift;
    const uint8_t *mask = c->masked ? c->active : nullptr;
    double omw = pl.omw;
    unsigned *flags = c->res_flags, *abort_flag = c->res_abort;
    std::lock_guard<std::mutex> lock(g_res_mu);
    hipError_t e = resident_chain_begin(c);
    if (e != hipSuccess) return e;
    if (pl.impl == 1) {
        // chained streaming passes: the dealt tiles, one wave each, flags by table slot
        unsigned *miss = reinterpret_cast<unsigned *>(c->tb_dealt + c->tb_dealt_miss_at);
        hipLaunchKernelGGL(STREAMING_CHAIN[2 * pl.fma + pl.guard], dim3(pl.tblocks), dim3(256), 0, c->stream, lut, code, xa, xb, nx, ny,
                           img_stride, dom_lo, own_lo, own_h, ntx, allb, nrows, shift, omw, pl.dealt, pl.nbrs, miss, npass, flags, base,
                           abort_flag, stamps);
        e = hipPeekAtLastError();
        if (e != hipSuccess) return e;
        c->tb_dealt_waves += (int64_t)pl.tblocks * 4;
        return resident_chain_end(c);
    }
    hipLaunchKernelGGL(pl.tile->kernel, dim3(pl.tblocks), dim3(pl.tile->threads()), 0, c->stream, lut, code, xa,
                       xb, nx, ny, img_stride, dom_lo, own_lo, own_h, cpi, ly, mask, ntx, gy, xmajor, allb, nrows, shift,
                       omw, npass, flags, base, abort_flag, xbytes, stall_tile, stamps);
    e = hipPeekAtLastError();
    if (e != hipSuccess) return e;
    return resident_chain_end(c);
}

// Did a resident launch give up?  Reads the flag (one 4-byte copy + a stream synchronisation) only when such a launch was
// enqueued since the last look.  A raised flag means some tile stopped updating -- another process's kernels held part of
// the chip, a CU mask -- and what the buffers hold is not a Jacobi iterate.  Nothing is lost: the field the interval started
// from was copied aside in front of its first resident launch (enqueue_sweeps), so the interval is redone from that copy
// with one launch per pass, and the context keeps launching that way (the condition that starved the tiles is not ours
// to lift).  The caller sees the same bits it would have seen; deff_get_plan("tb_fallbacks") counts the occurrences.
int resident_check(deff_ctx *c)
{
    if (!c->res_pending) return DEFF_OK;
    unsigned h = 0;
    HIP_TRY(hipMemcpyAsync(&h, c->res_abort, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->res_pending = false;
    const int64_t redo = c->res_redo;
    c->res_redo = 0;
    if (!h) return DEFF_OK;
    HIP_TRY(hipMemsetAsync(c->res_abort, 0, sizeof h, c->stream));
    c->tb_resident = 0;
    ++c->res_fallbacks;
    c->tb_debug_stall = 0;
    if (!c->res_backup) {
        c->have_field = false;
        return fail(DEFF_EHIP, "resident passes aborted and no restart copy exists (the field is invalid)");
    }
    HIP_TRY(hipMemcpyAsync(c->x[c->res_backup_cur], c->res_backup, sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
    c->cur = c->res_backup_cur;
    SweepPlan pl;
    TRY(plan_sweeps(c, c->res_omega, &pl));
    const int64_t launches = c->last_launches;
    TRY(enqueue_sweeps(c, pl, redo));
    c->last_launches = launches;                                   // (the redone launches are not the caller's)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}

static int pick_R(int requested, int dflt)
{
    const int r = requested ? requested : dflt;
    return r >= 8 ? 8 : r >= 4 ? 4 : r >= 2 ? 2 : 1;
}

static void tile_grid(const deff_ctx *c, int cols_per_block, int rows, SweepPlan *pl)
{
    pl->rows = rows;
    pl->gx = (c->nx + cols_per_block - 1) / cols_per_block;
    pl->cpi = (c->ny + rows - 1) / rows;               // row tiles never straddle two images
    pl->gy = pl->cpi * c->nimg;
    const unsigned total = (unsigned)pl->gx * (unsigned)pl->gy;
    pl->blocks = (int)(((total + 7u) / 8u) * 8u);      // see xcd_tile()
}

// Which form of the temporally blocked pass a context gets when the caller does not say (tb_impl = 0): workgroup tiles
// (kernels_wgtile.hpp) below 4 Mi cells in the context -- one image or a stack --, where the streaming kernel has too few
// tiles to fill the chip and a tile's dependency chain sets the time of a pass; everything larger streams.  Measured,
// G cells*iter/s, streaming / workgroup tiles: one image 512^2 106 / 231, 1024^2 316 / 556, 1536^2 455 / 613, 2048^2
// 682 / 678, 4096^2 1 128 / 742; stacks 16 x 128^2 117 / 239, 64 x 128^2 364 / 683, 200 x 128^2 589 / 652, 16 x 256^2
// 322 / 418, 48 x 256^2 535 / 535, 12 x 512^2 509 / 618, 2 x 1024^2 426 / 569, 3 x 1024^2 577 / 623 (and 1 024 x 128^2,
// 16 Mi cells, whole images per wave with no halo: 1 222 streaming).
// Since the resident forms (k_sweep_wgres) the numbers above are those of ONE LAUNCH PER PASS; with all tiles on the chip
// one image runs at 512^2 306, 1024^2 840-855 (8-wave tiles), 1536^2 835-866, 2048^2 933-958, 2304^2 958-966 (tall tiles,
// which plan_sweeps() also takes just above this threshold when they fit), 2 x 1024^2 958, 16 x 512^2 998.
// Keyed on tb_ref_cells for slabs, so that every slab of an image takes the same decision (and the same T).
int default_tb_impl(const deff_ctx *c)
{
    const size_t cells = c->tb_ref_cells ? c->tb_ref_cells : c->n;
    return cells < ((size_t)1 << 22) ? 2 : 1;
}

int default_tb_T(const deff_ctx *c)
{
    // workgroup tiles: 8 sweeps per pass amortise the launch gap and the first-load latency (1024^2: T = 8 556, T = 4 457)
    // (the pre-scaled arithmetic streams at every size: its T is the streaming form's, as with tb_impl = 1)
    if (!c->prescaled && (c->tb_impl ? c->tb_impl : default_tb_impl(c)) == 2) return 8;
    // streaming: below 4 Mi cells the launch is latency-bound and T = 4 wins; above, T = 8 everywhere (with the
    // prefetch really in flight, kernels_tb.hpp, stacks no longer prefer T = 6: 1 024 x 128^2 1 222 vs
    // 1 125 G cells*iter/s, 64 x 1024^2 1 258 vs 1 156, 16 x 1024^2 1 106 vs 1 064)
    const size_t cells = c->tb_ref_cells ? c->tb_ref_cells : c->n;
    return cells < ((size_t)1 << 22) ? 4 : 8;
}

// the instantiated sweeps-per-pass: 1, 2, 4, 6, 8 (one helper for the planner and deff_last_launches)
int clamp_tb_T(int T) { return T >= 8 ? 8 : T >= 6 ? 6 : T >= 4 ? 4 : T >= 2 ? 2 : 1; }

namespace deff {

// Is the system behind (dictionary, codes) link-symmetric the way wgl_sweeps' short-cut (kernels_wgtile.hpp) needs it?  For every cell: the E link
// of an even column equals, bit for bit, the W link of the odd column next to it (a lane's two cells), and the N link of a
// row equals the S link of the row above it in the same image.  The native assemblies are (fvm_row: a face has one
// harmonic mean); a dictionary harvested from somebody's matrix need not be.  Raises *flag on the first mismatch.
__global__ __launch_bounds__(256) void k_links_symmetric(const double *__restrict__ lut_g, const uint16_t *__restrict__ code,
                                                         int nx, int rows, int ny, int nrows, unsigned *flag)
{
    __shared__ double lut[LUT_DOUBLES];
    load_lut(lut, lut_g, nrows);
    constexpr int PS = LUT_PLANE_STRIDE * 8;
    const size_t n = (size_t)nx * rows;
    bool bad = false;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const int r = (int)(p / nx), c = (int)(p - (size_t)r * nx);
        const char *me = reinterpret_cast<const char *>(lut) + code[p];
        if (!(c & 1) && c + 1 < nx) {
            const char *east = reinterpret_cast<const char *>(lut) + code[p + 1];
            bad |= __double_as_longlong(*reinterpret_cast<const double *>(me + 2 * PS)) !=
                   __double_as_longlong(*reinterpret_cast<const double *>(east + PS));
        }
        if (r % ny != 0) {
            const char *north = reinterpret_cast<const char *>(lut) + code[p - nx];
            bad |= __double_as_longlong(*reinterpret_cast<const double *>(me + 4 * PS)) !=
                   __double_as_longlong(*reinterpret_cast<const double *>(north + 3 * PS));
        }
    }
    if (bad) atomicOr(flag, 1u);
}

}  // namespace deff

// Runs k_links_symmetric on the current (dictionary, codes) unless that was done since they last changed; the answer is
// c->links_sym (1 yes, 2 no).  Needs c->res_abort (its flag word) and synchronises the stream.
static int check_links_symmetric(deff_ctx *c)
{
    if (c->links_sym != 0) return DEFF_OK;
    unsigned h = 1;
    TRY(resident_check(c));                                        // the abort word doubles as this kernel's flag: read it first
    if (!c->res_abort) {
        TRY(dev_alloc(&c->res_abort, 1));
        HIP_TRY(hipMemsetAsync(c->res_abort, 0, sizeof(unsigned), c->stream));
    }
    unsigned *flag = c->res_abort;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_links_symmetric, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, c->lut, c->code, c->nx, c->rows,
                       c->ny, c->lut_nrows, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, flag, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->links_sym = h ? 2 : 1;
    return DEFF_OK;
}

// ---- the plan of a temporally blocked pass (T sweeps), piece by piece ------------------------------------------------

// Strips of 128 columns overlapping by 2*HW; a mesh wall needs no halo (kernels_tb.hpp).
// Placement A: every strip carries its halo, also outside the first column; placement B: no halo outside a wall.  B needs
// fewer strips for narrow images (a 128-column image is ONE strip: 2x on dataset batches); where the counts tie, A measured
// equal or up to 5 % faster in one process (T = 8 at 4096^2), so B is used only when it wins.
static void plan_strips(const deff_ctx *c, int T, SweepPlan *pl)
{
    const int hw = (T + 1) & ~1, wout = TB_COLS - 2 * hw;
    const int ntx_a = (c->nx + wout - 1) / wout;
    const int ntx_b = c->nx <= TB_COLS ? 1 : (c->nx - TB_COLS + wout - 1) / wout + 1;
    const bool use_b = c->tb_wall_halo == 0 ? true : (c->tb_wall_halo == 1 ? false : ntx_b < ntx_a);
    pl->shift = use_b ? 0 : hw;
    pl->ntx = use_b ? ntx_b : ntx_a;
}

// flags (one 256-byte block per tile) and the abort word of the resident launches.  A flag holds the number of passes its
// tile has completed since the array was last cleared (c->res_epoch, compared through a signed difference in the kernel):
// a new array starts a new count, and so does an old one before the count could wrap (launch_resident_passes).
static int ensure_resident_buffers(deff_ctx *c, long tiles)
{
    if (c->res_flags_n < (size_t)tiles) {
        TRY(resident_check(c));                                     // nothing resident may still be using the old array
        if (c->res_flags) { HIP_TRY(hipFree(c->res_flags)); c->res_flags = nullptr; }
        TRY(dev_alloc(&c->res_flags, (size_t)tiles * WGR_FLAG_STRIDE));
        HIP_TRY(hipMemsetAsync(c->res_flags, 0, sizeof(unsigned) * tiles * WGR_FLAG_STRIDE, c->stream));
        c->res_flags_n = (size_t)tiles;
        c->res_epoch = 0;
    }
    if (!c->res_abort) {
        TRY(dev_alloc(&c->res_abort, 1));
        HIP_TRY(hipMemsetAsync(c->res_abort, 0, sizeof(unsigned), c->stream));
    }
    return DEFF_OK;
}

// Can this plan run resident at all?  A whole context (a slab's halo rows change between passes from outside), not a band
// of one, 32-bit buffer offsets, and the caller has not asked for one launch per pass.
static bool resident_allowed(const deff_ctx *c, const SweepPlan *pl)
{
    return c->tb_resident && !c->slab && pl->band_h <= 0 && !pl->T_override && c->n * sizeof(double) < ((size_t)1 << 31);
}

// Row tiles a tall-tile image of own_h rows needs at R rows per wave.  A tall tile carries no halo rows beyond a wall of
// the mesh (its rows start at the image's first row, kernels_wgtile.hpp), so ONE tile holds 16R rows, two tiles 16R - T
// each, three or more 16R - 2T (the inner ones).  A 128^2 image of a stack is one tile of 16 x 8 rows: nothing recomputed,
// nobody to wait for.
static int wgl_row_tiles(int own_h, int R, int T)
{
    const int rows = WGL_WAVES * R;
    if (own_h <= rows) return 1;
    if (own_h <= 2 * (rows - T)) return 2;
    const int lymax = rows - 2 * T;
    return (own_h + lymax - 1) / lymax;
}

// THE row-tiling rule of the workgroup tiles, for every fit test and every plan.  An image of own_h rows on tiles of kernel t:
// `cpi` row tiles by the most rows a tile may own -- its rows less T rows of halo above and below; a tall tile as said above; a
// caller's tb_LY (8-wave tiles) when that is less --, the rows spread evenly over them, `LY` each, which `tcpi` <= cpi tiles
// hold.  A fit test counts cpi tiles per image, a plan launches tcpi.
struct RowTiles { int cpi, LY, tcpi; };
static RowTiles row_tiles(const TileKernel &t, int own_h, int tb_LY = 0)
{
    const int lymax = t.tile_rows() - 2 * t.T;
    RowTiles rt;
    rt.cpi = t.NW == WGL_WAVES ? wgl_row_tiles(own_h, t.R, t.T) : (own_h + lymax - 1) / lymax;
    if (tb_LY > 0 && tb_LY < lymax) rt.cpi = (own_h + tb_LY - 1) / tb_LY;
    rt.LY = (own_h + rt.cpi - 1) / rt.cpi;
    rt.tcpi = (own_h + rt.LY - 1) / rt.LY;
    return rt;
}

static long round_up_8(long tiles) { return ((tiles + 7) / 8) * 8; }                 // (a grid is whole XCD rounds, see xcd_tile())

// ... and the grid of a plan with these row tiles: one workgroup per tile.  Returns the tiles.
static long set_tile_grid(const deff_ctx *c, SweepPlan *pl, const RowTiles &rt)
{
    pl->LY = rt.LY;
    pl->tcpi = rt.tcpi;
    pl->tgy = rt.tcpi * c->nimg;
    const long tiles = (long)pl->ntx * pl->tgy;
    pl->tgx = (int)tiles;
    pl->tblocks = (int)round_up_8(tiles);
    return tiles;
}

// ---- candidates.  Nothing below changes the context or the device: a fit test asks (the occupancy of the kernel it would
// launch, remembered per kernel; once a 12-wave or tall candidate stands, whether the links are symmetric, remembered in
// c->links_sym), and a plan_<form> fills in a SweepPlan.  plan_blocked_pass puts them in order and gives the one it takes
// its buffers.

// The kernel of a tall tile of R rows per wave: rows dealt by age where TILES_TALL has a set for R and the system is unguarded
// (tuning "tb_tall_deal"), the 7-lookup short-cut when `sym` (the system is verified link-symmetric) and unguarded.
static const TileKernel *tall_tile(const deff_ctx *c, int R, bool fma, bool sym)
{
    const bool guard = c->lut_guard;
    const TileKernel *t = nullptr;
    if (c->tb_tall_deal && !guard)
        t = find_tile([&](const TileKernel &e) { return e.NW == WGL_WAVES && e.R == R && e.fma == fma && e.sym == sym && e.aged(); });
    if (!t)
        t = find_tile([&](const TileKernel &e) {
            return e.NW == WGL_WAVES && e.R == R && e.fma == fma && e.guard == guard && e.sym == (sym && !guard) && !e.aged();
        });
    return t;
}

static int set_tall_tile(const deff_ctx *c, SweepPlan *pl, int R, bool sym)
{
    pl->tile = tall_tile(c, R, pl->fma, sym);
    return pl->tile ? DEFF_OK : fail(DEFF_ESTATE, "internal: no tall-tile kernel of %d rows per wave", R);
}

// Tall resident tiles (16 waves x R rows, kernels_wgtile.hpp): the smallest R of TILES_TALL whose tiles all fit the chip -- or
// whose tiles are whole images, which wait for nobody and may queue for the CUs in any number --, or 0.  T = 8 only; not when
// the caller shapes the 8-wave tiles (tb_R, tb_LY) or insists on them (tb_NW = 8).
static int choose_tall_R(const deff_ctx *c, const SweepPlan *pl, int T, int own_h, int *tall_R)
{
    *tall_R = 0;
    if (T != 8 || !resident_allowed(c, pl) || c->tb_NW == WGT_WAVES || c->tb_NW == WGS_WAVES) return DEFF_OK;
    if (c->tb_NW != WGL_WAVES && (c->tb_R != 0 || c->tb_LY != 0)) return DEFF_OK;
    const bool caller_R = c->tb_NW == WGL_WAVES && tall_tile(c, c->tb_R, pl->fma, false);
    for (const TileKernel &t : TILES_TALL) {
        if (t.aged() || t.sym || t.fma != pl->fma || t.guard != c->lut_guard) continue;   // each R once
        if (caller_R && t.R != c->tb_R) continue;
        const int cpi = row_tiles(t, own_h).cpi;
        // the occupancy of the kernel plan_tall launches (whether the system is link-symmetric is only known there: the
        // short-cut kernels have the same, tests/test_kernel_resources.py)
        const TileKernel *k = tall_tile(c, t.R, pl->fma, false);
        int res = 0;
        TRY(resident_blocks(c, k->kernel, k->threads(), &res));
        const bool whole_images = pl->ntx == 1 && cpi == 1;
        if (round_up_8((long)pl->ntx * cpi * c->nimg) <= res || whole_images) { *tall_R = t.R; break; }
    }
    return DEFF_OK;
}

// 8-wave tiles (matrix rows in registers): rows per wave, rows per tile, grid; resident when all tiles fit the chip.
static int plan_tiles8(const deff_ctx *c, SweepPlan *pl, int T, int own_h)
{
    pl->impl = 2;
    auto tile8 = [&](const TileKernel &t) { return t.T == T && t.fma == pl->fma && t.guard == c->lut_guard; };
    // workgroups of a launch per pass: the caller's, or what the chip holds at once (at least one per CU)
    auto launched_at_once = [&](const TileKernel &t, int *res) -> int {
        *res = c->tb_wg;
        if (*res) return DEFF_OK;
        TRY(resident_blocks(c, t.pass, t.threads(), res));
        if (*res < 1) TRY(cu_count(c, res));
        return DEFF_OK;
    };
    const TileKernel *tile = find_tile([&](const TileKernel &t) { return t.NW == WGT_WAVES && tile8(t) && t.R == c->tb_R; });
    if (!tile) {
        // rows per wave: the fewest (shortest sweeps) whose tiles are all resident at once; if none is, 6
        // (7 needs 256 VGPRs and a few spilled registers: fine for one round, slower over several)
        tile = find_tile([&](const TileKernel &t) { return t.NW == WGT_WAVES && tile8(t) && t.R == 6; });
        for (const TileKernel &t : TILES_8WAVE) {
            if (!tile8(t)) continue;
            int res = 0;
            TRY(launched_at_once(t, &res));
            if ((long)pl->ntx * row_tiles(t, own_h).cpi * c->nimg <= res) { tile = &t; break; }
        }
    }
    if (!tile) return fail(DEFF_ESTATE, "internal: no 8-wave tile kernel for T = %d", T);
    pl->tile = tile;
    // rows a tile owns: at most 8R - 2T; spread the image's rows evenly over its row tiles
    const long tiles = set_tile_grid(c, pl, row_tiles(*tile, own_h, c->tb_LY));
    int at_once = 0;
    TRY(launched_at_once(*tile, &at_once));
    if (pl->tblocks > at_once) pl->tblocks = at_once >= 8 ? at_once / 8 * 8 : 8;
    // Resident passes (k_sweep_wgres): every tile on the chip at once, tiles at least T rows tall (a tile's halo must end
    // inside its immediate neighbours: they are the ones it waits for)
    pl->resident = false;
    if (resident_allowed(c, pl) && (pl->LY >= T || pl->tcpi == 1)) {
        int res = 0;
        TRY(resident_blocks(c, tile->kernel, tile->threads(), &res));
        if (round_up_8(tiles) <= res) {
            pl->resident = true;
            pl->tblocks = (int)round_up_8(tiles);
        }
    }
    return DEFF_OK;
}

// Tall tiles with R rows per wave: always resident; the 7-lookup short-cut when the system is verified link-symmetric.
static int plan_tall(deff_ctx *c, SweepPlan *pl, int own_h, int R)
{
    pl->impl = 2;
    pl->resident = true;
    if (c->tb_sym != 2) TRY(check_links_symmetric(c));            // once per (codes, dictionary): one pass over the codes
    TRY(set_tall_tile(c, pl, R, c->tb_sym != 2 && c->links_sym == 1));
    set_tile_grid(c, pl, row_tiles(*pl->tile, own_h));
    return DEFF_OK;
}

// Link-symmetric 12-wave tiles (k_sweep_wgsym): matrix rows in registers at 3 waves per SIMD.  A tile of 12 x R rows has the
// shape of an 8-wave tile of 1.5 R rows and sweeps it faster (three waves of a SIMD issue FP64 every ~5 clocks, two every ~6),
// so wherever the system is verified link-symmetric and unguarded this form replaces the 8-wave tiles: the first shape of
// TILES_12WAVE for this T (fewest rows first) whose tiles all fit the chip.  *sym = null: not applicable (not symmetric, guarded,
// too many tiles, caller insists on another form).  T = 8, 6, 4; resident launches only.
// The shapes with a row less for the younger waves (k_sweep_wgsage: a SIMD serves its three waves oldest first, and a tile's
// waves meet at a barrier in every sweep -- see k_sweep_wgage) are candidates for T = 8 unless tb_sym_age = 0.
static int choose_sym_tile(deff_ctx *c, const SweepPlan *pl, int T, int own_h, const TileKernel **sym)
{
    *sym = nullptr;
    if ((T != 8 && T != 6 && T != 4) || !resident_allowed(c, pl) || c->lut_guard || c->tb_sym == 2) return DEFF_OK;
    if (c->tb_NW != 0 && c->tb_NW != WGS_WAVES) return DEFF_OK;
    if (T != 8 && c->tb_T && c->tb_NW != WGS_WAVES) return DEFF_OK;  // a caller's T = 4 / 6 means these tiles only together with tb_NW = 12
    if (c->tb_NW != WGS_WAVES && (c->tb_R != 0 || c->tb_LY != 0)) return DEFF_OK;
    const bool t8 = T == 8 && c->tb_sym_age;
    const bool caller_R = c->tb_NW == WGS_WAVES && find_tile([&](const TileKernel &t) { return t.NW == WGS_WAVES && t.R == c->tb_R && !t.aged(); });
    const TileKernel *found = nullptr;
    int k = 0;
    for (const TileKernel &t : TILES_12WAVE) {
        if (t.T != T || t.fma != pl->fma || (t.aged() && !t8)) continue;
        ++k;
        if (caller_R && (t.R != c->tb_R || t.aged())) continue;          // a caller's R: equal rows of that many
        if (t8 && c->tb_sym_shape && k != c->tb_sym_shape) continue;     // tests: this shape of T = 8's list or none
        const RowTiles rt = row_tiles(t, own_h);
        if (rt.LY < T && rt.cpi > 1) continue;                      // a tile's halo must end inside its immediate neighbours
        int res = 0;
        TRY(resident_blocks(c, t.kernel, t.threads(), &res));
        if (round_up_8((long)pl->ntx * rt.cpi * c->nimg) <= res) { found = &t; break; }
    }
    if (!found) return DEFF_OK;
    TRY(check_links_symmetric(c));                                  // once per (codes, dictionary): one pass over the codes
    if (c->links_sym == 1) *sym = found;
    return DEFF_OK;
}

static void plan_sym(const deff_ctx *c, SweepPlan *pl, int own_h, const TileKernel *tile)
{
    pl->impl = 2;
    pl->tile = tile;
    pl->resident = true;
    set_tile_grid(c, pl, row_tiles(*tile, own_h));
}

// Streaming form: rows per chunk.  Workgroups are persistent, so a pass takes `rounds` tiles per wave slot (one round = as
// many wave tiles as are resident at once), and a tile costs its LY rows + T steps that drain the pipeline + T rows of halo
// above it unless it starts at the top wall of its image + a fixed start-up (first loads, measured ~8 row steps).  Pick the
// chunks per image minimising rounds x tile cost; for k rounds only the largest chunk count that fits matters.  (Stacks of
// small images: 3 072 x 128^2 as whole-image tiles 1 266 G cells*iter/s against 1 107 G for the 4 x 32-row tiles a
// halo-blind model picks.)
// Chunk heights by service order.  A SIMD serves the waves it holds oldest first (tools/tb_stamps.py: with equal chunks the
// three waves of a SIMD end at 71 / 89 / 108 us of a 4096^2 pass -- the SIMD runs on two waves, then on one, for a third of the
// launch), and which wave is the oldest is known beforehand: workgroups go to the XCDs round-robin and fill an XCD's CUs
// once around before any CU gets its second one (observed on every SIMD of the chip: workgroup (blockIdx >> 3) / 32 of an XCD
// = wave slot 0, 1, 2).  So the chunks need not be equal: the oldest rank gets the tallest, the youngest the shortest, in
// proportion to the speeds the ranks run at (tb_rank_w), and all three end together.  Each strip is cut into nq chunks
// per rank -- the oldest rank's at the top, the youngest's at the bottom --, a workgroup's four waves hold four stacked
// chunks of one rank, and an XCD's workgroups hold neighbouring strips (its L2 sees the shared halo rows).  The result
// is written as a table the kernel reads (k_sweep_matfree_tb, `dealt`); every row is still covered once, so the bits
// cannot change -- if the dispatch order is ever different (another process on the GPU), only the balance is lost.
static int deal_ranked_tiles(deff_ctx *c, SweepPlan *pl, int T, int own_lo, int own_h, int resident, bool *dealt)
{
    *dealt = false;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int xcds = 8, per_xcd = cus / xcds, occ = cus > 0 ? resident / cus : 0;
    if (cus % xcds != 0 || occ != 3 || resident != occ * cus) return DEFF_OK;       // three waves per SIMD is what was measured
    const int slots = cus * 4;                                                       // waves per rank
    const int ntx = pl->ntx, cap = own_h / (3 * T);
    const int ncol = ntx * c->nimg;                      // columns to cut into chunks: every strip of every image of a stack
    if (ntx > 0xFFFF || c->nimg > 0x7FFF || ncol > slots) return DEFF_OK;
    const int nq = std::min(slots / ncol, cap);
    if (nq < 1 || c->tb_rank_wall < 1000 || c->tb_rank_w[0] < 1 || c->tb_rank_w[1] < 1 || c->tb_rank_w[2] < 1) return DEFF_OK;
    const std::vector<int> key = {T, own_lo, own_h, ntx, c->nimg, pl->shift, resident, c->tb_rank_w[0], c->tb_rank_w[1], c->tb_rank_w[2], c->tb_rank_wall};
    auto fill_plan = [&]() {
        pl->dealt = c->tb_dealt;
        pl->LY = c->tb_dealt_LY;
        pl->tcpi = 3 * c->tb_dealt_nmax;                                             // (the stamps' numbering: rank, image, strip, chunk < nmax)
        pl->tgy = pl->tcpi * c->nimg;
        pl->tgx = (ntx * pl->tgy + 3) / 4;
        pl->tblocks = resident;
        pl->nbrs = c->tb_chain_fits ? c->tb_chain_nbrs : nullptr;
        *dealt = true;
    };
    if (c->tb_dealt && key == c->tb_dealt_key) { fill_plan(); return DEFF_OK; }
    const double v[3] = {(double)c->tb_rank_w[0], (double)c->tb_rank_w[1], (double)c->tb_rank_w[2]};
    const int K = T * (T - 1) + 8;                        // level steps a chunk costs on top of T per row: halo triangles + fill
    // A wall strip's waves look up b as well and run 10-15 % longer per row (mean end of a 4096^2 pass by strip, equal chunk
    // counts: 107 us in the first strip against 94...100 in the others): its rows count tb_rank_wall per mille.  A last strip
    // that is partly outside the mesh (4096 columns: half of it) moves fewer cache lines: the surcharge in proportion.
    // (the surcharge differs by rank: the oldest wave runs at the pace of its own dependency chain and pays every extra lookup --
    // its wall chunks ended 12-14 % after the rank's mean --, the youngest waits for issue slots anyway: 6 %)
    std::vector<std::array<double, 3>> speed(ncol, std::array<double, 3>{v[0], v[1], v[2]});
    const bool walls = ntx >= 3;
    if (walls) {
        const int hw = (T + 1) & ~1, wout = TB_COLS - 2 * hw;
        const int last_cols = c->nx - ((ntx - 1) * wout - pl->shift);                // columns of the last strip inside the mesh
        const double extra = c->tb_rank_wall / 1000.0 - 1.0, by_rank[3] = {2.5, 1.5, 1.0};
        const double fill = (double)std::min(last_cols, TB_COLS) / TB_COLS;
        for (int img = 0; img < c->nimg; ++img)
            for (int r = 0; r < 3; ++r) {
                speed[(size_t)img * ntx][r] = v[r] / (1.0 + extra * by_rank[r]);
                speed[(size_t)img * ntx + ntx - 1][r] = v[r] / (1.0 + extra * by_rank[r] * fill);
            }
    }
    // chunks per strip and rank: nq each, then the wave slots left over go one by one to the strip that would end last
    // (time of a strip = its level steps over the speed of its waves: (T own_h + K sum n_r) / sum n_r v_r)
    struct Strip { int n[3]; int ly[3]; };
    std::vector<Strip> st(ncol);
    for (auto &q : st) q.n[0] = q.n[1] = q.n[2] = nq;
    int spare[3] = {slots - ncol * nq, slots - ncol * nq, slots - ncol * nq};
    auto strip_time = [&](int tx) {
        const Strip &q = st[tx];
        const std::array<double, 3> &u = speed[tx];
        return ((double)T * own_h + (double)K * (q.n[0] + q.n[1] + q.n[2])) / (q.n[0] * u[0] + q.n[1] * u[1] + q.n[2] * u[2]);
    };
    for (int it = 0; it < 3 * slots; ++it) {
        int worst = -1;
        double tw = 0;
        for (int tx = 0; tx < ncol; ++tx) {
            const double t = strip_time(tx);
            if (t > tw) { tw = t; worst = tx; }
        }
        int r = -1;
        for (int k = 0; k < 3; ++k)
            if (spare[k] > 0 && st[worst].n[k] < cap && (r < 0 || spare[k] > spare[r])) r = k;
        if (r < 0) break;
        ++st[worst].n[r];
        --spare[r];
    }
    // chunk heights: a rank's chunk gets the rows its waves finish in the strip's time; the oldest rank takes the rounding
    int nmax = 0;
    for (int tx = 0; tx < ncol; ++tx) {
        Strip &q = st[tx];
        const double t = strip_time(tx);
        int left = own_h;
        for (int r = 2; r >= 1; --r) {
            int ly = (int)((t * speed[tx][r] - K) / T);
            if (ly < T) ly = T;
            q.ly[r] = ly;
            left -= q.n[r] * ly;
        }
        q.ly[0] = (left + q.n[0] - 1) / q.n[0];
        if (q.ly[0] < T) return DEFF_OK;
        nmax = std::max(nmax, std::max(q.n[0], std::max(q.n[1], q.n[2])));
    }
    if ((long)3 * c->nimg * ntx * nmax >= (1L << 30)) return DEFF_OK;
    int tallest = 0;                                              // rows of the tallest chunk dealt (tb_window_fits below)
    int shortest = INT32_MAX;                                     // ... and of the shortest that has any (deff_get_plan "tb_chunk_min")
    const size_t entries = (size_t)resident * 4 + 1;              // + the word the waves count their misplacements in (kernels_tb.hpp)
    {
        std::vector<int4> &tab = c->tb_dealt_host;
        tab.assign(entries, make_int4(0, 0, 0, 0));
        auto tile = [&](int r, int col, int q) {
            const Strip &sp = st[col];
            const int img = col / ntx, tx = col % ntx;
            const int own0 = own_lo + img * c->ny;                                  // (c->ny: the row pitch of a stack's images)
            const int own_hi = own0 + own_h;
            int ry0 = own0;
            for (int k = 0; k < r; ++k) ry0 += sp.n[k] * sp.ly[k];
            ry0 += q * sp.ly[r];
            int rows_here = std::min(sp.ly[r], own_hi - ry0);
            if (r == 2 && q == sp.n[2] - 1) rows_here = own_hi - ry0;              // the youngest rank's last chunk takes what rounding left over
            tallest = std::max(tallest, rows_here);
            if (rows_here > 0) shortest = std::min(shortest, rows_here);
            return make_int4(tx | (img << 16), ry0, rows_here > 0 ? rows_here : 0, (int)((unsigned)(((r * c->nimg + img) * ntx + tx) * nmax + q) | ((unsigned)r << 30)));
        };
        for (int r = 0; r < 3; ++r) {
            // workgroup m of rank r: XCD m / per_xcd, the (m % per_xcd)-th of that XCD's workgroups of this rank
            auto slot = [&](int m, int w) { return ((((size_t)(r * per_xcd + m % per_xcd) << 3) | (size_t)(m / per_xcd)) * 4 + w); };
            std::vector<char> used((size_t)cus * 4, 0);
            // the wall strips' chunks first, one per workgroup and spread over the chip (twelve waves looking up b on one CU
            // were the last to end by 5 us), each rank starting elsewhere
            std::vector<int4> wall_tiles;
            if (walls)
                for (int img = 0; img < c->nimg; ++img)
                    for (int tx : {0, ntx - 1})
                        for (int q = 0; q < st[(size_t)img * ntx + tx].n[r]; ++q) wall_tiles.push_back(tile(r, img * ntx + tx, q));
            const int nw = (int)wall_tiles.size();
            for (int k = 0; k < nw; ++k) {
                int m = (int)(((long)k * cus) / std::max(nw, 1) + (long)r * cus / 3) % cus, w = 0;
                while (used[(size_t)m * 4 + w]) { if (++w == 4) { w = 0; m = (m + 1) % cus; } }
                used[(size_t)m * 4 + w] = 1;
                tab[slot(m, w)] = wall_tiles[k];
            }
            // the inner strips in order (chunk index fastest): a workgroup's waves hold stacked chunks, an XCD neighbouring strips
            int m = 0, w = 0;
            for (int col = 0; col < ncol; ++col) {
                if (walls && (col % ntx == 0 || col % ntx == ntx - 1)) continue;
                for (int q = 0; q < st[col].n[r]; ++q) {
                    while (m < cus && used[(size_t)m * 4 + w]) { if (++w == 4) { w = 0; ++m; } }
                    if (m >= cus) return fail(DEFF_ESTATE, "dealt tiles: more chunks than waves (rank %d)", r);
                    used[(size_t)m * 4 + w] = 1;
                    tab[slot(m, w)] = tile(r, col, q);
                }
            }
        }
        // (the kernel's 32-bit row offsets; a table that fails is not uploaded and equal chunks, checked in turn, take over)
        if (!tb_window_fits(c->nx, tallest, T)) return DEFF_OK;
        if (c->tb_dealt_cap < entries) {
            TRY(resident_check(c));
            if (c->tb_dealt) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->tb_dealt)); c->tb_dealt = nullptr; }
            HIP_TRY(hipMalloc((void **)&c->tb_dealt, entries * sizeof(int4)));
            c->tb_dealt_cap = entries;
        }
        HIP_TRY(hipMemcpyAsync(c->tb_dealt, tab.data(), entries * sizeof(int4), hipMemcpyHostToDevice, c->stream));
        // who waits for whom if this table's passes are chained (tb_chain.hpp: from the geometry, by rectangle intersection);
        // uploaded beside the table as slot + 1, 0 = none.  A table whose lists do not fit is not chained.
        std::vector<int> lists;
        const TbChainGeom geom{c->nx, T, pl->shift, ntx, c->ny, c->dom_lo, c->mesh_ny, own_lo, own_h};
        c->tb_chain_fits = tb_chain_lists(geom, reinterpret_cast<const TbChainTile *>(tab.data()), entries - 1, &lists);
        std::vector<unsigned> up(lists.size());
        if (c->tb_chain_fits) {
            for (size_t k = 0; k < lists.size(); ++k) up[k] = (unsigned)(lists[k] + 1);
            if (c->tb_chain_nbrs_cap < up.size()) {
                if (c->tb_chain_nbrs) { HIP_TRY(hipFree(c->tb_chain_nbrs)); c->tb_chain_nbrs = nullptr; }   // (nothing in flight: resident_check above or a first table)
                HIP_TRY(hipMalloc((void **)&c->tb_chain_nbrs, up.size() * sizeof(unsigned)));
                c->tb_chain_nbrs_cap = up.size();
            }
            HIP_TRY(hipMemcpyAsync(c->tb_chain_nbrs, up.data(), up.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));                                   // (pageable sources; once per plan change)
        c->tb_dealt_key = key;
        c->tb_dealt_LY = st[ntx / 2].ly[1];
        c->tb_dealt_min = shortest == INT32_MAX ? 0 : shortest;
        c->tb_dealt_max = tallest;
        c->tb_dealt_nmax = nmax;
        c->tb_dealt_miss_at = (size_t)resident * 4;
        c->tb_dealt_waves = 0;
        c->tb_dealt_looks = 0;
    }
    fill_plan();
    return DEFF_OK;
}

// Where chained passes are the default.  Measured against the parent build (profiles/r06_tb_chain_ab.log):
// one 4096^2 image (16 Mi cells, a pass of ~100 us) +2.7 %; 8192^2 and 64 x 1024^2 (64 Mi cells, passes of ~430 us) -2...-5 %
// -- a launch boundary is worth ~9 us + the tail whatever the size, the tiles' waits and the coherent rows cost in
// proportion to the pass.  Nothing was measured between the two, so the rule stops at what won.
static bool chain_pays(const deff_ctx *c)
{
#ifdef TB_CHAIN_ALWAYS                                  // (measurement switch: chain every dealt plan; never set by the Makefile)
    return c->n > 0;
#else
    return c->n <= ((size_t)1 << 24);
#endif
}

static int plan_streaming(deff_ctx *c, SweepPlan *pl, int T, int own_lo, int own_h)
{
    pl->impl = 1;
    pl->resident = false;
    pl->chained = false;
    pl->nbrs = nullptr;
    pl->guard = c->lut_guard;                          // the reference's non-zero link test matters only when a phase cannot diffuse
    int resident = c->tb_wg;
    if (!resident) {
        if (pl->pre) TRY(resident_blocks(c, STREAMING_PRE[tb_index(T)], 256, &resident));
        else TRY(resident_blocks(c, STREAMING[tb_index(T)][2 * pl->fma + pl->guard], 256, &resident));
        if (resident < 1) TRY(cu_count(c, &resident));                // at least one workgroup per CU
    }
    pl->dealt = nullptr;
    // (T = 8 only: the ranks' speeds were measured there; with them T = 6 gains 3 % at 4096^2 and loses 4 % at 8192^2)
    if (c->tb_ranked && !c->tb_rank_lost && !c->tb_LY && !c->tb_wg && pl->band_h == 0 && !c->slab && T == 8 && !c->masked) {
        bool dealt = false;
        TRY(deal_ranked_tiles(c, pl, T, own_lo, own_h, resident, &dealt));
        // chained passes: on the conditions of the resident tiles (a whole context, 32-bit offsets, the caller has not asked
        // for one launch per pass, no earlier fallback) when the neighbour lists fit and where it was measured to win
        // (the pre-scaled form is not chained: one launch per pass)
        if (dealt) pl->chained = !pl->pre && pl->nbrs && c->tb_chain && resident_allowed(c, pl) && chain_pays(c);
        if (pl->chained) {
            // every wave of the grid must be on the chip for the whole launch: by the chained kernel's own occupancy
            int at_once = 0;
            TRY(resident_blocks(c, STREAMING_CHAIN[2 * pl->fma + pl->guard], 256, &at_once));
            if (at_once < pl->tblocks) pl->chained = false;
        }
        if (dealt) return DEFF_OK;
    }
    int LY = c->tb_LY;
    if (!LY) {
        long best_cost = -1;
        const bool top_wall = own_lo == 0;              // not a slab with rows above it
        for (int k = 1; k <= 8; ++k) {
            const int cpi_max = (int)(((long)k * resident * 4) / ((long)pl->ntx * c->nimg));
            if (cpi_max < 1) continue;
            int ly = (own_h + cpi_max - 1) / cpi_max;
            // chunks shorter than the pipeline is deep lose more to fill/drain than the model says (1024^2, T=4: 3-row
            // chunks 254 G, 4..6-row chunks 295 G cells*iter/s)
            if (ly < T) ly = T;
            const int cpi = (own_h + ly - 1) / ly;
            const long cost = (long)k * (ly + T + ((cpi > 1 || !top_wall) ? T : 0) + 8);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; LY = ly; }
        }
        if (!LY) LY = own_h;
    }
    if (LY > own_h) LY = own_h;
    // The streaming kernel addresses a chunk's rows through 32-bit buffer offsets from the chunk's own window (tb_strip,
    // kernels_tb.hpp): (LY + 2 T) rows x nx doubles must stay below 2 GiB, the offset that marks a lane as outside.  A chunk
    // that could not fit (a quarter of a million cells per row and more, times a tall chunk) is not launched: the context
    // sweeps with the single-sweep matrix-free kernel, as contexts too small for a blocked pass do.
    if (!tb_window_fits(c->nx, LY, T)) { pl->kernel = DEFF_KERNEL_MATFREE; return DEFF_OK; }
    pl->LY = LY;
    pl->tcpi = (own_h + LY - 1) / LY;
    pl->tgy = pl->tcpi * c->nimg;
    pl->tgx = (int)(((long)pl->ntx * pl->tgy + 3) / 4);           // workgroup tiles (4 wave tiles each)
    const unsigned total = (unsigned)pl->tgx;
    pl->tblocks = (int)(((total + 7u) / 8u) * 8u);
    if (pl->tblocks > resident) pl->tblocks = resident >= 8 ? resident / 8 * 8 : 8;
    return DEFF_OK;
}

// what deff_get_plan() reports: the plan of whole passes of the context (not a slab's T = 1 remainder plan, not a band)
static void record_plan(deff_ctx *c, const SweepPlan *pl)
{
    if (pl->band_h > 0 || (pl->impl != 2 && pl->T_override)) return;
    c->plan_T = pl->T; c->plan_LY = pl->LY; c->plan_ntx = pl->ntx; c->plan_cpi = pl->tcpi;
    c->plan_blocks = pl->tblocks; c->plan_impl = pl->impl;
    c->plan_R = pl->impl == 2 ? pl->tile->R : 0;
    c->plan_NW = pl->impl == 2 ? pl->tile->NW : 0;
    c->plan_resident = pl->impl == 2 && pl->resident ? 1 : 0;
    c->plan_ranked = pl->impl == 1 && pl->dealt ? 1 : 0;
    c->plan_chain = pl->impl == 1 && pl->chained ? 1 : 0;
    c->plan_aged = pl->impl == 2 && pl->tile->aged() ? 1 : 0;
}

// The workgroup-tile form of a pass of T sweeps, in the order of DESIGN.md section 4, "What the planner picks": each candidate
// either does not apply / does not fit, or is the plan.  Decides only (see "candidates" above).
static int choose_tile_form(deff_ctx *c, SweepPlan *pl, int T, int own_h, int tall_R)
{
    // 1. Images that are ONE tall tile each (a stack of 128^2 images) recompute nothing and wait for nobody: nothing beats that.
    if (tall_R && pl->ntx == 1 && wgl_row_tiles(own_h, tall_R, T) == 1) {
        if (c->tb_NW != WGT_WAVES) return plan_tall(c, pl, own_h, tall_R);
    } else {
        // 2. 12-wave tiles against resident 8-wave tiles.  Both coefficient-resident forms may fit the chip: a sweep costs a SIMD
        // its share of the tile's rows times the clocks a row takes at that occupancy -- measured (tools/wgr_stamps.py) ~160 at
        // two waves per SIMD, ~142 at three.  512^2 / 640^2 stay on 8 waves x 4 rows (303-476 G against 310-481 G on 12 x 3,
        // which is therefore not instantiated), 768^2 ... 1100^2 go to 12 waves (559 against 511 G, 746 against 688 G, 850
        // against 808 G).
        const TileKernel *sym = nullptr;
        TRY(choose_sym_tile(c, pl, T, own_h, &sym));
        if (sym && c->tb_NW != WGS_WAVES) {
            SweepPlan alt = *pl;
            TRY(plan_tiles8(c, &alt, T, own_h));
            if (alt.resident && 2 * alt.tile->R * 160 <= 3 * sym->R * 142) { *pl = alt; return DEFF_OK; }
        }
        if (sym) { plan_sym(c, pl, own_h, sym); return DEFF_OK; }
    }
    // (the caller asked for 12-wave tiles at this T: those or nothing)
    if (c->tb_NW == WGS_WAVES && (T == 6 || T == 4) && c->tb_T)
        return fail(DEFF_EINVAL, "tb_T = %d on 12-wave tiles: the tiles are not co-resident or the system is not link-symmetric", T);
    // 3. 8-wave tiles, all resident (a caller's tb_NW = 16 takes tall tiles that fit first)
    SweepPlan tiles8 = *pl;
    TRY(plan_tiles8(c, &tiles8, T, own_h));
    if (tiles8.resident && !(tall_R && c->tb_NW == WGL_WAVES)) { *pl = tiles8; return DEFF_OK; }
    // 4. Images a little too large for the 12-wave tiles at T = 8 (1101 ... 1172 columns: 1152^2 is 297 tiles of 44 x 112
    // owned cells) fit with passes of SIX sweeps -- 48 x 116 owned cells per tile, 240 tiles at 1152^2 -- and a sweep
    // then costs (6 x 5 rows x 3 waves x ~142 clocks + the exchange) / 6 = ~3 300 clocks against ~4 000 ... 4 800 on
    // tall tiles (lookups in every sweep, 4 waves per SIMD): taken whenever it fits and the caller has fixed neither T
    // nor the form.
    // Passes of FOUR (52 x 120 owned cells: up to 1208 columns x 1248 rows) come after that: ~4 200 clocks per sweep,
    // still ahead of the tall tiles' ~4 900 where those need R = 5.
    if (!tiles8.resident && T == 8 && !c->tb_T && (c->tb_NW == 0 || c->tb_NW == WGS_WAVES) && !c->tb_R && !c->tb_LY) {
        for (int Ts : {6, 4}) {
            SweepPlan alt = *pl;
            alt.T = Ts;
            plan_strips(c, Ts, &alt);
            const TileKernel *rs = nullptr;
            TRY(choose_sym_tile(c, &alt, Ts, own_h, &rs));
            if (Ts == 4 && rs && rs->R < 5 && tall_R && tall_R <= 4) rs = nullptr;      // (4 x 4 rows per sweep: no better than tall R = 4)
            if (rs) { plan_sym(c, &alt, own_h, rs); *pl = alt; return DEFF_OK; }
        }
    }
    // 5. tall tiles
    if (tall_R) return plan_tall(c, pl, own_h, tall_R);
    // 6. 8-wave tiles, one launch per pass
    *pl = tiles8;
    return DEFF_OK;
}

// The form of a blocked pass ("What the planner picks"): the first workgroup-tile form whose tiles are all
// resident; else 8-wave tiles with one launch per pass below 4 Mi cells and streaming above.  The form is decided first;
// then the plan that was taken, and no other, gets its buffers on the device.
static int plan_blocked_pass(deff_ctx *c, SweepPlan *pl)
{
    // sweeps per pass (measured, G cells*iter/s: 4096^2 T=4 926, T=6 1063, T=8 1106; stacks of 16 x 1024^2 peak at T=6;
    // 1024^2 alone at T=4)
    const int T = clamp_tb_T(pl->T_override ? pl->T_override : (c->tb_T ? c->tb_T : default_tb_T(c)));
    pl->T = T;
    // rows this plan updates: the context's owned rows, or a band of them (row slabs split a pass into the bands the
    // neighbours wait for and the interior, api_slab.hip)
    const int own_lo = pl->band_h > 0 ? pl->band_lo : c->own_lo;
    const int own_h = pl->band_h > 0 ? pl->band_h : c->own_h;
    pl->own_lo = own_lo;
    pl->own_h = own_h;
    plan_strips(c, T, pl);
    int tall_R = 0;
    if (!pl->pre) TRY(choose_tall_R(c, pl, T, own_h, &tall_R));
    int want_impl = c->tb_impl ? c->tb_impl : default_tb_impl(c);
    // the pre-scaled arithmetic exists on the streaming form alone: taken at every size, as tb_impl = 1 would
    if (pl->pre) want_impl = 1;
    // a context just above the 4 Mi cells where the streaming form takes over still runs faster on tall tiles when they fit
    if (!c->tb_impl && want_impl == 1 && tall_R) want_impl = 2;
    // workgroup tiles exist for T = 4 and 8 (the 12-wave link-symmetric form also for T = 6, on request); slabs' T = 1 remainder
    // passes and the other T stay on the streaming kernel
    if (want_impl == 2 && (T == 4 || T == 8 || (T == 6 && c->tb_NW == WGS_WAVES)) && !pl->T_override) {
        TRY(choose_tile_form(c, pl, T, own_h, tall_R));
        if (pl->resident) TRY(ensure_resident_buffers(c, (long)pl->ntx * pl->tgy));
    } else {
        TRY(plan_streaming(c, pl, T, own_lo, own_h));
        if (pl->kernel != DEFF_KERNEL_MATFREE_TB) return DEFF_OK;     // (a chunk window the kernel cannot address: single sweeps)
        if (pl->chained) TRY(ensure_resident_buffers(c, (long)pl->tblocks * 4));    // one flag per wave of the grid
    }
    record_plan(c, pl);
    return DEFF_OK;
}

int plan_sweeps(deff_ctx *c, double omega, SweepPlan *pl)
{
    if (!c->have_field) return fail(DEFF_ESTATE, "no field: call deff_init_linear() or deff_set_field()");
    // an explicit system (host-assembled, 3-phase, ImpSolid) with few distinct rows also runs matrix-free
    if (c->kernel == DEFF_KERNEL_AUTO || c->kernel == DEFF_KERNEL_MATFREE || c->kernel == DEFF_KERNEL_MATFREE_TB)
        TRY(ensure_dictionary(c));
    TRY(resolve_kernel(c, &pl->kernel));
    // The pre-scaled arithmetic (tuning "prescaled"): matrix-free sweeps only, refused here -- before the field, the system or
    // the recorded plan are touched -- for everything else.  `fma` is ignored by the sweeps while it is set.
    pl->pre = c->prescaled != 0;
    if (pl->pre) {
        if (c->slab) return fail(DEFF_EINVAL, "prescaled: not for row-slab contexts");
        if (c->kernel == DEFF_KERNEL_EXPLICIT || c->kernel == DEFF_KERNEL_SCALAR)
            return fail(DEFF_EINVAL, "prescaled: the explicit and scalar kernels have no pre-scaled form (deff_set_kernel: auto, matfree or matfree_tb)");
        if (pl->kernel != DEFF_KERNEL_MATFREE && pl->kernel != DEFF_KERNEL_MATFREE_TB)
            return fail(DEFF_EINVAL, "prescaled: the system has no row dictionary (the pre-scaled sweeps are matrix-free)");
    }
    pl->fma = c->fma != 0 && !pl->pre;
    pl->omega = omega;
    pl->omw = 1.0 - omega;                              // cuh:89 evaluates (1.0 - w) in double
    if (pl->kernel == DEFF_KERNEL_MATFREE || pl->kernel == DEFF_KERNEL_MATFREE_TB) {
        TRY(upload_lut(c, omega));
        if (pl->pre) {
            if (c->lut_guard)
                return fail(DEFF_EINVAL, "prescaled: the row dictionary has a singular row (a phase that cannot diffuse): "
                                         "omega / A0 is not finite there and the table cannot be pre-scaled");
            TRY(upload_lut_pre(c, omega));
        }
        if (pl->kernel == DEFF_KERNEL_MATFREE_TB) TRY(plan_blocked_pass(c, pl));
        // single sweeps (the first sweep and the n mod T remainder): 4 rows per tile and up to 8 192 workgroups (measured at
        // 4096^2: 52.0 us = 5.8 TB/s against 59-61 us for 8 rows x 2 048 persistent workgroups; 16384^2: 960-990 us = 4.9-5.0
        // TB/s either way -- above what a plain copy kernel gets from HBM for this read / write mix, tools/ubench mem: 4.7 TB/s)
        tile_grid(c, 256 * 2, pick_R(c->rows_matfree, c->n >= ((size_t)1 << 21) ? 4 : 2), pl);
        // persistent grid: workgroups walk the tiles (tables loaded once each)
        const int cap = c->wg_matfree ? c->wg_matfree : 256 * 32;
        if (pl->blocks > cap) pl->blocks = cap;
    } else {
        TRY(explicit_from_image(c));
        if (c->c0_omega != omega) {
            hipLaunchKernelGGL(k_make_c0, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->a0, omega, c->c0,
                               c->n);
            HIP_TRY(hipGetLastError());
            c->c0_omega = omega;
        }
        if (pl->kernel == DEFF_KERNEL_EXPLICIT)
            tile_grid(c, 512, pick_R(c->rows_explicit, 1), pl);
    }
    c->plan_prescaled = pl->pre ? 1 : 0;                // deff_get_plan "prescaled": the arithmetic of the sweeps this plan runs
    return DEFF_OK;
}

// A stream has put new images into slots (deff_solve_stream): what the plan took from the codes before is looked at again.
int replan_for_new_codes(deff_ctx *c, double omega, SweepPlan *pl)
{
    // the explicit / scalar kernels read coefficient planes, not codes: assemble them again with the new images' rows
    if ((pl->kernel == DEFF_KERNEL_EXPLICIT || pl->kernel == DEFF_KERNEL_SCALAR) && !c->have_explicit) {
        *pl = SweepPlan();
        TRY(plan_sweeps(c, omega, pl));
    }
    // new images, new codes: the symmetric short-cut of the tall tiles is re-verified, not carried over
    if (pl->impl == 2 && pl->tile->NW == WGL_WAVES && c->tb_sym != 2 && c->links_sym == 0) {
        TRY(check_links_symmetric(c));
        TRY(set_tall_tile(c, pl, pl->tile->R, c->links_sym == 1));
    } else if (pl->impl == 2 && pl->tile->NW == WGS_WAVES && c->links_sym == 0) {
        TRY(check_links_symmetric(c));
        if (c->links_sym != 1) { *pl = SweepPlan(); TRY(plan_sweeps(c, omega, pl)); }   // (never for the native assembly)
    }
    return DEFF_OK;
}

// Single sweeps (kernels_sweep.hpp), [2 nt + fma] and, by rows per tile 1, 2, 4, 8, [rows_index(rows)][...]
static constexpr auto SCALAR_SWEEPS = by_flags([](auto nt, auto f) { return k_sweep_scalar<decltype(nt)::value, decltype(f)::value>; });
template <int... R> static constexpr auto explicit_sweeps()
{
    return std::array{by_flags([](auto nt, auto f) { return k_sweep_explicit<R, decltype(nt)::value, decltype(f)::value>; })...};
}
template <int... R> static constexpr auto matfree_sweeps()
{
    return std::array{by_flag([](auto f) { return k_sweep_matfree<2, R, decltype(f)::value>; })...};
}
static constexpr auto EXPLICIT_SWEEPS = explicit_sweeps<1, 2, 4, 8>();
static constexpr auto MATFREE_SWEEPS = matfree_sweeps<1, 2, 4, 8>();
static constexpr std::array MATFREE_SWEEPS_PRE = {k_sweep_matfree_pre<1>, k_sweep_matfree_pre<2>, k_sweep_matfree_pre<4>, k_sweep_matfree_pre<8>};
static int rows_index(int rows) { return rows == 1 ? 0 : rows == 2 ? 1 : rows == 4 ? 2 : 3; }

// Enqueue one sweep x[cur] -> x[cur^1] and flip (the reference copies instead, cuh:1281).
void enqueue_sweep(deff_ctx *c, const SweepPlan &pl)
{
    const double *xin = c->x[c->cur];
    double *xout = c->x[c->cur ^ 1];
    const CoefConst cf{c->c0, c->aW, c->aE, c->aS, c->aN, c->b};
    const int flip = c->serpentine ? c->cur : 0;
    const uint8_t *mask = c->masked ? c->active : nullptr;
    const int nt = c->nt_explicit ? 2 : 0;
    switch (pl.kernel) {
    case DEFF_KERNEL_SCALAR:
        hipLaunchKernelGGL(SCALAR_SWEEPS[nt + pl.fma], dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, cf, xin, xout,
                           c->nx, c->n, c->n_img, mask, pl.omw);
        break;
    case DEFF_KERNEL_EXPLICIT:
        hipLaunchKernelGGL(EXPLICIT_SWEEPS[rows_index(pl.rows)][nt + pl.fma], dim3(pl.blocks), dim3(256), 0, c->stream, cf, xin, xout,
                           c->nx, c->ny, c->rows, pl.cpi, mask, pl.gx, pl.gy, flip, pl.omw);
        break;
    default:
        if (pl.pre) {
            hipLaunchKernelGGL(MATFREE_SWEEPS_PRE[rows_index(pl.rows)], dim3(pl.blocks), dim3(256), 0, c->stream, c->lut_pre, c->code, xin,
                               xout, c->nx, c->ny, c->rows, pl.cpi, mask, pl.gx, pl.gy, flip, c->lut_nrows, pl.omw);
            break;
        }
        hipLaunchKernelGGL(MATFREE_SWEEPS[rows_index(pl.rows)][pl.fma], dim3(pl.blocks), dim3(256), 0, c->stream, c->lut, c->code, xin,
                           xout, c->nx, c->ny, c->rows, pl.cpi, mask, pl.gx, pl.gy, flip, c->lut_nrows, pl.omw);
        break;
    }
    c->cur ^= 1;
}

// Is the chip dispatching the way the dealt tiles assume?  Called where the stream has just been synchronised, for the first
// three such points after a table was built: the waves that found themselves in another slot than their tile was cut for have
// counted themselves (kernels_tb.hpp).  More than a quarter of them misplaced -- somebody else's kernels on the GPU, another
// dispatch order -- and the context goes back to equal chunks; the results are the same bits either way.
int dealt_watch(deff_ctx *c)
{
    if (!c->tb_dealt || c->tb_dealt_looks >= 3 || c->tb_dealt_waves == 0) return DEFF_OK;
    unsigned miss = 0;
    HIP_TRY(hipMemcpyAsync(&miss, reinterpret_cast<const char *>(c->tb_dealt + c->tb_dealt_miss_at), sizeof miss, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->tb_dealt_looks;
    c->tb_rank_misses = (int)std::min<int64_t>(miss, INT32_MAX);
    if ((int64_t)miss * 4 > c->tb_dealt_waves) c->tb_rank_lost = 1;
    return DEFF_OK;
}

// One temporally blocked pass: T sweeps, x[cur] -> x[cur^1].
int enqueue_tb_pass(deff_ctx *c, const SweepPlan &pl)
{
    TRY(launch_tb_pass(c, pl));
    c->cur ^= 1;
    return DEFF_OK;
}

// The launch of a pass (or of one band of it: pl.own_lo / pl.own_h) without the buffer flip.
int launch_tb_pass(deff_ctx *c, const SweepPlan &pl)
{
    const double *xin = c->x[c->cur];
    double *xout = c->x[c->cur ^ 1];
    const int flip = c->serpentine ? c->cur : 0;
    const uint8_t *mask = c->masked ? c->active : nullptr;
    const int allb = (c->lut_allb || c->nx != c->nxt) ? 1 : 0;       // padded: the wall column may not be in the last strip
    if (pl.impl == 2) {
        if (!pl.tile->pass)
            return fail(DEFF_ESTATE, "tiles of %d waves only exist as resident launches (plan again with tb_launch = 1)", pl.tile->NW);
        hipLaunchKernelGGL(pl.tile->pass, dim3(pl.tblocks), dim3(pl.tile->threads()), 0, c->stream, c->lut, c->code, xin, xout, c->nx,
                           c->mesh_ny, c->ny, c->dom_lo, pl.own_lo, pl.own_h, pl.tcpi, pl.LY, mask, pl.ntx, pl.tgy, c->tb_xmajor, allb,
                           c->lut_nrows, pl.shift, pl.omw, c->tb_stamps);
        HIP_TRY(hipPeekAtLastError());
        return DEFF_OK;
    }
    if (pl.pre) {
        // the same tiles over the pre-scaled table; b' is looked up everywhere unless it is +0.0 wherever b is zero
        const int allb_pre = (allb || c->lut_pre_allb) ? 1 : 0;
        hipLaunchKernelGGL(STREAMING_PRE[tb_index(pl.T)], dim3(pl.tblocks), dim3(256), 0, c->stream, c->lut_pre, c->code, xin, xout,
                           c->nx, c->mesh_ny, c->ny, c->dom_lo, pl.own_lo, pl.own_h, pl.tcpi, mask, pl.LY, pl.ntx, pl.tgx, pl.tgy, flip,
                           c->tb_xmajor, allb_pre, c->lut_nrows, pl.shift, pl.omw, c->tb_stamps, pl.dealt);
        HIP_TRY(hipPeekAtLastError());
        if (pl.dealt) c->tb_dealt_waves += (int64_t)pl.tblocks * 4;
        return DEFF_OK;
    }
    hipLaunchKernelGGL(STREAMING[tb_index(pl.T)][2 * pl.fma + pl.guard], dim3(pl.tblocks), dim3(256), 0, c->stream, c->lut, c->code,
                       xin, xout, c->nx, c->mesh_ny, c->ny, c->dom_lo, pl.own_lo, pl.own_h, pl.tcpi, mask, pl.LY, pl.ntx, pl.tgx, pl.tgy,
                       flip, c->tb_xmajor, allb, c->lut_nrows, pl.shift, pl.omw, c->tb_stamps, pl.dealt);
    HIP_TRY(hipPeekAtLastError());
    if (pl.dealt) c->tb_dealt_waves += (int64_t)pl.tblocks * 4;
    return DEFF_OK;
}

// Passes one resident launch may hold: ~25 ms (a pass of T sweeps takes about n * T / 0.9e12 s on these forms), between 64 and 4 096.
static int64_t resident_pass_cap(const deff_ctx *c, const SweepPlan &pl)
{
    const double pass_s = (double)c->n * pl.T / 0.9e12;
    return std::max<int64_t>(64, std::min<int64_t>(4096, (int64_t)(25e-3 / pass_s)));
}

// (workgroup tiles, or the chained form of the streaming kernel)
// All whole passes of n sweeps as resident launches of up to 4 096 passes (tens of milliseconds each); *n is reduced by
// the sweeps enqueued.  In front of the first resident launch since the abort flag was last looked at, the field is copied
// aside: the restart point if a launch gives up (resident_check).
static int launch_resident_passes(deff_ctx *c, const SweepPlan &pl, int64_t *n)
{
    int64_t np = *n / pl.T;
    if (np > 0 && !c->res_pending) {
        TRY(dev_alloc(&c->res_backup, c->n));
        HIP_TRY(hipMemcpyAsync(c->res_backup, c->x[c->cur], sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
        c->res_backup_cur = c->cur;
        c->res_redo = 0;
        c->res_omega = pl.omega;
    }
    // a resident launch holds the whole chip until it ends: keep one to ~25 ms (a pass of T sweeps takes about n * T / 0.9e12 s
    // on these forms), between 64 and 4 096 passes -- the reference's 10 000-sweep interval is one launch up to ~1500^2
    const int64_t cap = resident_pass_cap(c, pl);
    while (np > 0) {
        const int chunk = (int)(np < cap ? np : cap);
        if (c->res_epoch > (1u << 30)) {
            // the flags count passes since they were last cleared and are compared through a signed difference: start a
            // new count long before it could wrap (stream-ordered: every earlier launch has finished with them)
            HIP_TRY(hipMemsetAsync(c->res_flags, 0, sizeof(unsigned) * c->res_flags_n * WGR_FLAG_STRIDE, c->stream));
            c->res_epoch = 0;
        }
        const hipError_t e = launch_resident(c, pl, c->x[c->cur], c->x[c->cur ^ 1], chunk, c->res_epoch);
        if (e != hipSuccess) return fail(DEFF_EHIP, "resident launch failed: %s", hipGetErrorString(e));
        c->res_epoch += (unsigned)chunk;
        c->res_pending = true;
        c->cur ^= (chunk & 1);
        np -= chunk;
        *n -= (int64_t)chunk * pl.T;
        c->res_redo += (int64_t)chunk * pl.T;
        c->last_launches += pl.impl == 1 ? chunk : 1;              // a chained launch counts its passes (deff_last_launches)
    }
    return DEFF_OK;
}

// n sweeps: as many T-sweep passes as fit, the rest one at a time.  Stops at the first launch that fails.
int enqueue_sweeps(deff_ctx *c, const SweepPlan &pl, int64_t n)
{
    // (a stack some of whose images have stopped since the plan was made -- deff_solve_batch keeps its plan -- goes on with one
    // launch per pass on the same table: that kernel leaves frozen images alone, a chain has no mask)
    const bool chained = pl.kernel == DEFF_KERNEL_MATFREE_TB && pl.impl == 1 && pl.chained && !c->masked;
    if (((pl.kernel == DEFF_KERNEL_MATFREE_TB && pl.impl == 2 && pl.resident) || chained) && !c->tb_resident) {
        // the context fell back to one launch per pass (resident_check) after this plan was made
        SweepPlan again;
        TRY(plan_sweeps(c, pl.omega, &again));
        if (again.resident || again.chained) return fail(DEFF_ESTATE, "internal: plan still resident after the fallback");
        return enqueue_sweeps(c, again, n);
    }
    // chained streaming passes: two passes or more go through the resident launches' machinery (a single pass gains nothing)
    if (chained && n >= 2 * pl.T) TRY(launch_resident_passes(c, pl, &n));
    // (while resident launches are in flight unchecked, whatever follows them is part of what a fallback must redo)
    if (pl.kernel == DEFF_KERNEL_MATFREE_TB && pl.impl == 2 && pl.resident && n >= (pl.tile->pass ? 2 : 1) * pl.T)
        TRY(launch_resident_passes(c, pl, &n));
    if (pl.kernel == DEFF_KERNEL_MATFREE_TB && !(pl.impl == 2 && !pl.tile->pass)) {
        while (n >= pl.T) { TRY(enqueue_tb_pass(c, pl)); n -= pl.T; ++c->last_launches; if (c->res_pending) c->res_redo += pl.T; }
    }
    for (; n > 0; --n) { enqueue_sweep(c, pl); ++c->last_launches; if (c->res_pending) ++c->res_redo; }
    HIP_TRY(hipPeekAtLastError());
    return DEFF_OK;
}

extern "C" int deff_sweeps(deff_ctx *c, int64_t nsweeps, double omega, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (nsweeps < 0) return fail(DEFF_EINVAL, "negative sweep count");
    TRY(use_device(c));
    SweepPlan pl;
    TRY(plan_sweeps(c, omega, &pl));
    TRY(consolidate(c));
    c->last_launches = 0;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    TRY(enqueue_sweeps(c, pl, nsweeps));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    TRY(resident_check(c));
    TRY(dealt_watch(c));
    return DEFF_OK;
}
DEFF_API_CATCH

// Diagnostics: time-stamp every wave tile of ONE temporally blocked pass (100 MHz wall clock ticks).
// out[2*k], out[2*k+1] = start, end of wave tile k; *ntiles = number of tiles (call with out = NULL
// to size the buffer; that call leaves the field alone).  Advances the field by one pass = T sweeps; by THREE passes =
// 3 * T sweeps when the plan is resident (workgroup tiles, "tb_resident" = 1), whose stamps cover three passes.
extern "C" int deff_debug_tb_stamps(deff_ctx *c, double omega, unsigned long long *out, int *ntiles)
try {
    if (!c || !ntiles) return fail(DEFF_EINVAL, "NULL argument");
    TRY(use_device(c));
    SweepPlan pl;
    TRY(plan_sweeps(c, omega, &pl));
    if (pl.kernel != DEFF_KERNEL_MATFREE_TB) return fail(DEFF_ESTATE, "not on the temporally blocked kernel");
    TRY(consolidate(c));
    // streaming form: 2 stamps per wave tile; workgroup-tile form: T + 4 per tile, flattened -- *ntiles is always
    // the number of PAIRS the buffer must hold
    // (resident launches stamp 12 clocks per tile whatever T: entry + 3 passes x {neighbours seen, halo in, swept, published})
    // (chained streaming launches: two header words, then TB_CHAIN_STAMPS clocks per tile -- entry, where, 3 passes x six
    // clocks, see k_sweep_matfree_tb_chain.  The caller writes the header into `out` before the call: out[0] = the first of the
    // three passes to stamp, out[1] = the passes of the chain, 0 meaning out[0] + 3; the field advances by that many passes.
    // The chain must be ONE launch -- see launch_resident_passes for how many passes that holds.)
    const bool chain_stamps = pl.impl == 1 && pl.chained;
    const bool res_stamps = (pl.impl == 2 && pl.resident) || chain_stamps;
    const int n = chain_stamps ? (TB_CHAIN_STAMP_HEAD + pl.ntx * pl.tgy * TB_CHAIN_STAMPS) / 2 : res_stamps ? (pl.ntx * pl.tgy * 12 + 1) / 2 : pl.impl == 2 ? (pl.ntx * pl.tgy * (pl.T + 4) + 1) / 2 : pl.ntx * pl.tgy;
    *ntiles = n;
    if (!out) return DEFF_OK;
    HIP_TRY(hipMalloc((void **)&c->tb_stamps, sizeof(unsigned long long) * 2 * n));
    HIP_TRY(hipMemsetAsync(c->tb_stamps, 0, sizeof(unsigned long long) * 2 * n, c->stream));
    int rc = DEFF_OK;
    int64_t passes = 3;
    if (chain_stamps) {
        const unsigned long long first = out[0];
        passes = out[1] ? (int64_t)out[1] : (int64_t)first + 3;
        if (first > 4093ull || passes < (int64_t)first + 3 || passes > resident_pass_cap(c, pl)) {
            (void)hipFree(c->tb_stamps);
            c->tb_stamps = nullptr;
            return fail(DEFF_EINVAL, "stamps of passes %llu ... + 2 of a chain of %lld: not one launch", first, (long long)passes);
        }
        HIP_TRY(hipMemcpyAsync(c->tb_stamps, out, sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                                          // (`out` is the caller's, pageable)
    }
    if (res_stamps) rc = enqueue_sweeps(c, pl, passes * pl.T);                                  // k_sweep_wgres / wgsym: 12 stamps per tile, 3 passes
    else rc = enqueue_tb_pass(c, pl);
    if (rc != DEFF_OK) { (void)hipFree(c->tb_stamps); c->tb_stamps = nullptr; return rc; }
    hipError_t e = hipMemcpyAsync(out, c->tb_stamps, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(c->tb_stamps);
    c->tb_stamps = nullptr;
    if (e != hipSuccess) return fail(DEFF_EHIP, "stamp readback failed: %s", hipGetErrorString(e));
    TRY(resident_check(c));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_last_launches(const deff_ctx *c, int64_t *launches, int *sweeps_per_pass)
try {
    if (!c || !launches) return fail(DEFF_EINVAL, "NULL argument");
    *launches = c->last_launches;
    if (sweeps_per_pass) {
        int k = 0;
        *sweeps_per_pass = 1;
        if (resolve_kernel(c, &k) == DEFF_OK && k == DEFF_KERNEL_MATFREE_TB) {
            *sweeps_per_pass = c->plan_T ? c->plan_T : clamp_tb_T(c->tb_T ? c->tb_T : default_tb_T(c));   // (the planner may take T = 6)
        }
    }
    return DEFF_OK;
}
DEFF_API_CATCH
