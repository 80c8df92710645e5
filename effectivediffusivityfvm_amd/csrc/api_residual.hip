// api_residual.hip -- deff_residual / deff_residual_D: the reference's Residual() (Deff2DGPU/Deff2D.cuh:451-494) of the
// context's current field, reduced on the device (kernels_residual.hpp).
#include "cell_pass.hpp"
#include "kernels_residual.hpp"
static_assert(RES_ROWS == CELL_PASS_ROWS && RES_COLS == CELL_PASS_COLS, "cell_pass_items plans the class kernel's tiles");

// (dy/dx) * H per class pair, the wall conductance and the "no face" zero -- the reference's expressions, evaluated once on
// the host (this file is built with -ffp-contract=off like the rest of the library)
static ResTable residual_table(const deff_ctx *c)
{
    ResTable t;
    const double dx = c->dx, dy = c->dy;
    for (int k = 0; k < 3; ++k) {
        for (int q = 0; q < 3; ++q) t.g[k][q] = dy / (dx) * whm(dx / 2, dx / 2, c->phase_D[k], c->phase_D[q]);   // cuh:469
        t.g[k][3] = dy / (dx / 2) * c->phase_D[k];                                                              // cuh:466
        for (int q = 4; q < 8; ++q) t.g[k][q] = 0.0;
    }
    return t;
}

// sums -> means: R / (numCols * numRows), cuh:491.  The residual's own event pair (pass_res), so a residual taken inside a
// solve loop's callback leaves the loop's ev0 / ev1 -- and with them loop_ms -- alone.
static int residual_finish(deff_ctx *c, const CellItems &it, double *r, float *ms)
{
    std::vector<double> sums(it.nimg);
    TRY(cell_pass_finish(c, c->pass_res, k_residual_final, it, sums.data(), nullptr, ms));
    const double cells = (double)((int64_t)c->nxt * (int64_t)c->ny);
    for (int k = 0; k < it.nimg; ++k) r[k] = sums[k] / cells;
    return DEFF_OK;
}

static int residual_common(deff_ctx *c, const double *r)
{
    if (!c || !r) return fail(DEFF_EINVAL, "NULL argument");
    if (c->slab) return fail(DEFF_EINVAL, "deff_residual: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    if (c->nxt < 2 || c->ny < 2) return fail(DEFF_EINVAL, "the residual needs a mesh of at least 2 x 2 cells");
    TRY(use_device(c));
    return DEFF_OK;
}

// the class kernel over `nimg` stacked images starting at field `x` / pixels `pix`; sums -> pass_res.part (after the partials)
static int residual_classes(deff_ctx *c, const double *x, const uint8_t *pix, int nimg, double *r, float *ms)
{
    if (!c->phase_mode || !c->have_image)
        return fail(DEFF_ESTATE, "deff_residual needs a system assembled from the image (deff_assemble_2phase / _3phase); "
                                 "pass the diffusivities to deff_residual_D() otherwise");
    if ((uint64_t)c->ny * (uint64_t)c->nx * 8u >= ((uint64_t)1 << 32))
        return fail(DEFF_EINVAL, "deff_residual: an image of more than 512 Mi cells (use deff_residual_D)");
    CellPass &p = c->pass_res;
    const CellItems it = cell_pass_items(c->nxt, c->ny, nimg, p.kt);
    TRY(cell_pass_room(c, p, false, it.items));
    const ResTable tab = residual_table(c);
    const bool fast = c->ampX == 1 && c->ampY == 1 && (c->W % 2) == 0;
    const dim3 grid((unsigned)((it.items + 3) / 4));
    TRY(cell_pass_start(c, p, ms));
#define LAUNCH_RES(P_, F_)                                                                                              \
    hipLaunchKernelGGL((k_residual_classes<P_, F_>), grid, dim3(256), 0, c->stream, x, pix, c->W, c->ampX,              \
                       c->ampY, c->nx, c->nxt, c->ny, nimg, it.ntx, it.cpi, it.kt, c->CL, c->CR, tab, p.part)
    if (c->phase_mode == 2) { if (fast) LAUNCH_RES(2, true); else LAUNCH_RES(2, false); }
    else { if (fast) LAUNCH_RES(3, true); else LAUNCH_RES(3, false); }
#undef LAUNCH_RES
    HIP_TRY(hipGetLastError());
    return residual_finish(c, it, r, ms);
}

extern "C" int deff_residual(deff_ctx *c, double *r, float *ms)
try {
    TRY(residual_common(c, r));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    return residual_classes(c, c->x[c->cur], c->pix, c->nimg, r, ms);
}
DEFF_API_CATCH

// One image of a stack, wherever its newest field lives (a frozen image of a batch solve, a slot of a running stream: callable
// from the deff_image_done_fn callback, like deff_get_slot_field).
extern "C" int deff_residual_slot(deff_ctx *c, int slot, double *r)
try {
    TRY(residual_common(c, r));
    if (slot < 0 || slot >= c->nimg) return fail(DEFF_EINVAL, "bad slot");
    TRY(resident_check(c));                                        // settled already inside the stream's callback: a no-op there
    const double *x = c->x[(c->masked || c->in_stream) ? c->buf_of[slot] : c->cur] + (size_t)slot * c->n_img;
    return residual_classes(c, x, c->pix + (size_t)slot * c->W * c->H, 1, r, nullptr);
}
DEFF_API_CATCH

extern "C" int deff_residual_D(deff_ctx *c, const double *D, double CL, double CR, double *r, float *ms)
try {
    TRY(residual_common(c, r));
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(consolidate(c));
    CellPass &p = c->pass_res;
    const int segs = (c->nxt + 255) / 256;
    const size_t per_img = (size_t)c->ny * segs;
    const CellItems it{segs, 0, c->ny, c->nimg, per_img, per_img * c->nimg};   // no runs (kt 0): one partial sum per row segment
    TRY(cell_pass_room(c, p, false, it.items));
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    TRY(cell_pass_start(c, p, ms));
    hipLaunchKernelGGL(k_residual_plane, dim3((unsigned)(c->rows * segs)), dim3(256), 0, c->stream, c->x[c->cur], dD, c->nx,
                       c->nxt, c->ny, c->nimg, segs, c->dx, c->dy, CL, CR, p.part);
    HIP_TRY(hipGetLastError());
    return residual_finish(c, it, r, ms);
}
DEFF_API_CATCH
