// api_fill.hip -- the flood fill of the pore space on the device (kernels_fill.hpp) and the native 3-phase assembly on top of
// it: deff_assemble_3phase_native, deff_get_grid.  The 3-phase counterpart of deff_assemble_2phase: pixels in, 16-bit row
// codes and an a-priori row table (row_index3.hpp) out; a continuation stage (same image, another Dg) rebuilds the table
// on the host and the wall diffusivities, nothing else.  See ctx.hpp for the file map.
#include "ctx.hpp"
#include "flood_fill.hpp"
#include "kernels_fill.hpp"
#include "row_index3.hpp"

static bool fill_fits_one_workgroup(const deff_ctx *c) { return (size_t)c->ny * fill_words(c->nxt) <= (size_t)FILL_LARGE_WORDS; }

// One image on the host (flood_fill.hpp): for the images the device forms cannot take or gave up on.
static int fill_on_host(deff_ctx *c, int img)
{
    const int nw = c->fill_nw, nx = c->nxt, ny = c->ny;
    std::vector<uint8_t> px((size_t)c->W * c->H);
    HIP_TRY(hipMemcpyAsync(px.data(), c->pix + (size_t)img * c->W * c->H, px.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<unsigned int> grid((size_t)nx * ny);
    for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j) grid[(size_t)i * nx + j] = px[(size_t)(i / c->ampY) * c->W + j / c->ampX] > 200 ? 1u : 0u;
    c->fill_path[img] = flood_fill(grid.data(), nx, ny);
    std::vector<uint64_t> open((size_t)ny * nw, 0), reach((size_t)ny * nw, 0);
    for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j) {
            const unsigned int g = grid[(size_t)i * nx + j];
            if (g != 1) open[(size_t)i * nw + (j >> 6)] |= 1ull << (j & 63);
            if (g == 0) reach[(size_t)i * nw + (j >> 6)] |= 1ull << (j & 63);
        }
    const size_t off = (size_t)img * ny * nw;
    HIP_TRY(hipMemcpyAsync(c->fill_open + off, open.data(), open.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->fill_reach + off, reach.data(), reach.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->fill_fallbacks;
    return DEFF_OK;
}

constexpr int FILL_BATCH = 8;                         // tile launches between two looks at the `changed` words

// The fill of the context's pixels into c->fill_reach, PathFlags into c->fill_path.
static int compute_fill(deff_ctx *c)
{
    const int nw = fill_words(c->nxt), nimg = c->nimg, ny = c->ny;
    const size_t words = (size_t)c->rows * nw;
    c->fill_nw = nw;
    TRY(dev_alloc(&c->fill_open, words));
    TRY(dev_alloc(&c->fill_reach, words));
    TRY(dev_alloc(&c->fill_status, (size_t)nimg * FILL_STATUS + 16));     // (+ the used-row bits of k_phase_codes3)
    c->fill_path.assign(nimg, 0);
    const int impl = c->fill_impl ? c->fill_impl : (fill_fits_one_workgroup(c) ? 1 : 2);
    std::vector<uint8_t> on_host(nimg, 0);
    int launches = 0;
    if (impl == 1) {
        const long long cap = fill_round_cap(ny, c->nxt);
        if ((size_t)ny * nw <= (size_t)FILL_SMALL_WORDS)
            hipLaunchKernelGGL((k_fill_image<FILL_SMALL_WORDS, FILL_SMALL_THREADS>), dim3(nimg), dim3(FILL_SMALL_THREADS), 0, c->stream,
                               c->pix, c->W, c->ampX, c->ampY, c->nxt, ny, nw, cap, c->fill_open, c->fill_reach, c->fill_status);
        else
            hipLaunchKernelGGL((k_fill_image<FILL_LARGE_WORDS, FILL_LARGE_THREADS>), dim3(nimg), dim3(FILL_LARGE_THREADS), 0, c->stream,
                               c->pix, c->W, c->ampX, c->ampY, c->nxt, ny, nw, cap, c->fill_open, c->fill_reach, c->fill_status);
        HIP_TRY(hipGetLastError());
        launches = 1;
    } else if (3 * (size_t)nw > (size_t)FILL_LARGE_WORDS) {
        // a row and its two halo rows do not fit a workgroup's LDS (more than 174 000 columns): every image on the host
        HIP_TRY(hipMemsetAsync(c->fill_status, 0, sizeof(int) * nimg * FILL_STATUS, c->stream));
        std::fill(on_host.begin(), on_host.end(), 1);
    } else {
        // rows per tile: the tuning key, else 16 .. ny / 128 (about 128 tiles for a large image: every compute unit gets
        // work, and a tile still crosses many rows per launch), clipped to what fits the LDS with the two halo rows
        const int tr_max = FILL_LARGE_WORDS / nw - 2;
        int tr = c->fill_tile_rows ? c->fill_tile_rows : std::max(16, (ny + 127) / 128);
        tr = std::max(1, std::min(std::min(tr, tr_max), ny));
        const int ntiles = (ny + tr - 1) / tr;
        const long long cap = fill_round_cap(tr, c->nxt);
        const int launch_cap = fill_launch_cap(ny, c->nxt);
        TRY(dev_alloc(&c->fill_changed, (size_t)(FILL_BATCH + 1) * nimg));
        hipLaunchKernelGGL(k_fill_open, dim3(grid_for(words * 64)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY,
                           c->nxt, ny, nw, nimg, c->fill_open, c->fill_reach, c->fill_status);
        HIP_TRY(hipGetLastError());
        ++launches;
        // changed[0][img]: the last launch of the batch before (all ones in front of the first), changed[k][img]: launch k
        HIP_TRY(hipMemsetAsync(c->fill_changed, 0xFF, sizeof(unsigned) * nimg, c->stream));
        std::vector<unsigned> last(nimg);
        int tile_launches = 0;
        for (;;) {
            HIP_TRY(hipMemsetAsync(c->fill_changed + nimg, 0, sizeof(unsigned) * nimg * FILL_BATCH, c->stream));
            for (int k = 1; k <= FILL_BATCH; ++k) {
                hipLaunchKernelGGL((k_fill_tiles<FILL_LARGE_WORDS, FILL_LARGE_THREADS>), dim3((unsigned)((size_t)ntiles * nimg)),
                                   dim3(FILL_LARGE_THREADS), 0, c->stream, c->fill_open, c->fill_reach, c->nxt, ny, nw, tr, ntiles, cap,
                                   c->fill_changed + (size_t)(k - 1) * nimg, c->fill_changed + (size_t)k * nimg, c->fill_status);
                HIP_TRY(hipGetLastError());
            }
            tile_launches += FILL_BATCH;
            HIP_TRY(hipMemcpyAsync(last.data(), c->fill_changed + (size_t)FILL_BATCH * nimg, sizeof(unsigned) * nimg,
                                   hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            bool done = true;
            for (int k = 0; k < nimg; ++k) done = done && last[k] == 0;
            if (done) break;
            if (tile_launches >= launch_cap) {                       // out of launches: what still changes goes to the host
                for (int k = 0; k < nimg; ++k) on_host[k] = last[k] != 0;
                break;
            }
            HIP_TRY(hipMemcpyAsync(c->fill_changed, c->fill_changed + (size_t)FILL_BATCH * nimg, sizeof(unsigned) * nimg,
                                   hipMemcpyDeviceToDevice, c->stream));
        }
        launches += tile_launches;
        hipLaunchKernelGGL(k_fill_path, dim3(nimg), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nxt, ny, nw,
                           c->fill_reach, c->fill_status);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    std::vector<int> st((size_t)nimg * FILL_STATUS);
    HIP_TRY(hipMemcpyAsync(st.data(), c->fill_status, sizeof(int) * st.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rounds = 0;
    for (int k = 0; k < nimg; ++k) {
        c->fill_path[k] = st[(size_t)k * FILL_STATUS];
        rounds = std::max(rounds, st[(size_t)k * FILL_STATUS + 2]);
        if (st[(size_t)k * FILL_STATUS + 1]) on_host[k] = 1;          // a workgroup ran into its round cap
    }
    for (int k = 0; k < nimg; ++k)
        if (on_host[k]) TRY(fill_on_host(c, k));
    c->fill_plan_impl = impl;
    c->fill_plan_launches = launches;
    c->fill_plan_rounds = rounds;
    ++c->fill_runs;
    c->fill_valid = true;
    c->codes3_valid = false;
    return DEFF_OK;
}

// Explicit SoA planes of the native 3-phase system, on demand like explicit_from_image's for two phases: D from the pixels,
// the Grid expanded from the bitmaps, then the general assembly (DiscretizeMatrix2D_ImpSolid).
int native3_explicit(deff_ctx *c)
{
    if (c->have_explicit) return DEFF_OK;
    if (!c->native3 || !c->fill_valid) return fail(DEFF_ESTATE, "no native 3-phase system assembled");
    TRY(ensure_explicit(c));
    TRY(ensure_scratch(c, (sizeof(double) + sizeof(unsigned int)) * c->n));
    double *D = (double *)c->scratch;
    unsigned int *G = (unsigned int *)((char *)c->scratch + sizeof(double) * c->n);
    hipLaunchKernelGGL(k_fill_D_3phase, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                       c->nxt, c->ny, c->rows, c->phase_D[0], c->phase_D[1], c->phase_D[2], D);
    hipLaunchKernelGGL(k_fill_grid, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx, c->nxt,
                       c->ny, c->rows, c->fill_reach, c->fill_nw, G);
    hipLaunchKernelGGL(k_assemble_from_D, dim3(grid_for(c->n)), dim3(256), 0, c->stream, D, G, c->nx, c->nxt, c->ny, c->rows,
                       c->dom_lo, c->mesh_ny, c->dx, c->dy, c->CL, c->CR, soa_of(c));
    HIP_TRY(hipGetLastError());
    c->have_explicit = true;
    c->c0_omega = NAN;
    c->wrap_links = false;
    return DEFF_OK;
}

extern "C" int deff_assemble_3phase_native(deff_ctx *c, double Ds, double Df, double Dg, double CL, double CR)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (c->slab)
        return fail(DEFF_EINVAL, "deff_assemble_3phase_native: not for row-slab contexts (the fill is a property of the whole image)");
    if (!c->have_image) return fail(DEFF_ESTATE, "deff_assemble_3phase_native needs an image");
    if (c->fill_impl == 1 && !fill_fits_one_workgroup(c))
        return fail(DEFF_EINVAL, "fill_impl 1: the bitmaps of a %d x %d image (%d words) do not fit one workgroup (%d words)", c->nxt,
                    c->ny, c->ny * fill_words(c->nxt), FILL_LARGE_WORDS);
    TRY(use_device(c));
    TRY(resident_check(c));                          // an unchecked resident interval is settled under the OLD field / system
    TRY(ensure_walls(c));
    if (!c->fill_valid) TRY(compute_fill(c));
    TRY(dev_alloc(&c->code, c->n));
    if (!c->codes3_valid) {
        unsigned *used = (unsigned *)(c->fill_status + (size_t)c->nimg * FILL_STATUS);
        HIP_TRY(hipMemsetAsync(used, 0, sizeof(unsigned) * 16, c->stream));
        hipLaunchKernelGGL(k_phase_codes3, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                           c->nxt, c->ny, c->rows, c->fill_reach, c->fill_nw, c->code, used);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->rows3_used, used, sizeof(unsigned) * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->codes3_valid = true;
    }
    c->CL = CL; c->CR = CR;
    hipLaunchKernelGGL(k_wall_D_3phase, dim3((c->rows + 255) / 256), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY,
                       c->nxt, c->ny, c->rows, Df, Ds, Dg, c->Dl, c->Dr);
    HIP_TRY(hipGetLastError());
    c->have_walls = true;
    // the table: what build_lut_rows is to the 2-phase system
    c->lut_nrows = NATIVE3_ROWS;
    c->lut_rows.resize((size_t)NATIVE3_ROWS * 6);
    build_rows3(c->lut_rows.data(), Ds, Df, Dg, c->dx, c->dy, CL, CR);
    // A row that no cell of this image has is made an identity row: with a phase that cannot diffuse (Ds = 0) the a-priori
    // table holds singular rows -- a pore cell walled in on every side, which the fill takes out of the system -- and a
    // singular row anywhere in the table would put every sweep on the guarded kernels (upload_lut).  A harvested
    // dictionary holds no such row either.
    for (int k = NATIVE3_FIRST; k < NATIVE3_ROWS; ++k)
        if (!(c->rows3_used[k >> 5] & (1u << (k & 31)))) {
            double *row = &c->lut_rows[(size_t)k * 6];
            row[0] = 1.0; row[1] = row[2] = row[3] = row[4] = row[5] = 0.0;
        }
    c->lut_allb = false;
    c->lut_omega = NAN;
    c->have_matfree = true;
    c->links_sym = 0;
    dict_reset(c);
    c->wrap_links = false;
    c->phase_mode = 3; c->phase_D[0] = Df; c->phase_D[1] = Ds; c->phase_D[2] = Dg;
    c->have_explicit = false;                        // built on demand (native3_explicit)
    c->native3 = true;
    adjoint_reset(c);
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_get_grid(deff_ctx *c, unsigned int *Grid, int *path_flag)
try {
    if (!c || (!Grid && !path_flag)) return fail(DEFF_EINVAL, "NULL argument");
    if (!c->fill_valid) return fail(DEFF_ESTATE, "no fill: deff_assemble_3phase_native() computes one for the current image");
    if (Grid) {
        TRY(use_device(c));
        TRY(ensure_scratch(c, sizeof(unsigned int) * c->n));
        unsigned int *G = (unsigned int *)c->scratch;
        hipLaunchKernelGGL(k_fill_grid, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx, c->nxt,
                           c->ny, c->rows, c->fill_reach, c->fill_nw, G);
        HIP_TRY(hipGetLastError());
        TRY(rows_d2h(c, Grid, (const unsigned int *)G, (size_t)c->rows));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (path_flag)
        for (int k = 0; k < c->nimg; ++k) path_flag[k] = c->fill_path[k];
    return DEFF_OK;
}
DEFF_API_CATCH
