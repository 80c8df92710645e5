// api_sens.hip -- deff_sensitivity / deff_sensitivity_D / deff_device_sensitivity: the per-cell gradient dDeff_raw / dD of the
// context's current field and its Euler sum, one pass on the device (kernels_sens.hpp).  Reads the field; changes nothing but
// the map, its partial sums and the shared upload scratch.
#include "ctx.hpp"
#include "kernels_sens.hpp"
#include <algorithm>
#include <vector>

// Everything that can refuse the call, before anything is touched.
static int sens_common(deff_ctx *c, const char *who, double CL, double CR)
{
    if (c->slab) return fail(DEFF_EINVAL, "%s: not for row-slab contexts (the rows of the image live on several devices)", who);
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    if (CR == CL) return fail(DEFF_EINVAL, "%s: CR == CL (Deff is a flux per unit of CR - CL)", who);
    TRY(use_device(c));
    return DEFF_OK;
}

// the map of the stack's newest fields (x[cur] after consolidate) for the D plane `dD` on the device (pitch nx, pad column 0)
static int sens_launch(deff_ctx *c, const double *dD, double CL, double CR, double *g, double *euler, float *ms)
{
    // work items as the residual's (api_residual.hip): column strips of 128, cut into runs of kt tiles of SENS_ROWS rows, about
    // 4 096 items in a launch and at most 16 384 per image; tuning "sens_kt" overrides
    const int ntx = (c->nxt + SENS_COLS - 1) / SENS_COLS, tiles_y = (c->ny + SENS_ROWS - 1) / SENS_ROWS;
    int kt = c->sens_kt;
    if (kt <= 0) {
        kt = (int)std::min<size_t>(64, std::max<size_t>(1, (size_t)ntx * tiles_y * c->nimg / 4096));
        kt = std::max(kt, (int)(((size_t)ntx * tiles_y + 16383) / 16384));
    }
    if (kt > tiles_y) kt = tiles_y;
    const int cpi = (tiles_y + kt - 1) / kt;
    const size_t per_img = (size_t)ntx * cpi, items = per_img * c->nimg;
    if ((items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_sensitivity: too many work items");
    TRY(dev_alloc(&c->sens_g, c->n));
    const size_t want = items + (size_t)c->nimg;
    if (c->sens_part_cap < want) {
        if (c->sens_part) { HIP_TRY(hipFree(c->sens_part)); c->sens_part = nullptr; c->sens_part_cap = 0; }
        HIP_TRY(hipMalloc((void **)&c->sens_part, want * sizeof(double)));
        c->sens_part_cap = want;
    }
    if (ms) {                                                      // the call's own pair: ev0 / ev1 belong to the solve loops
        if (!c->sens_ev0) HIP_TRY(hipEventCreate(&c->sens_ev0));
        if (!c->sens_ev1) HIP_TRY(hipEventCreate(&c->sens_ev1));
        HIP_TRY(hipEventRecord(c->sens_ev0, c->stream));
    }
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), den = (CR - CL) * (CR - CL);
    double *out = c->sens_part + items;
    hipLaunchKernelGGL(k_sens, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], dD, c->nx, c->nxt, c->ny,
                       c->nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, den, c->sens_g, c->sens_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sens_final, dim3(c->nimg), dim3(1024), 0, c->stream, c->sens_part, per_img, out);
    HIP_TRY(hipGetLastError());
    if (ms) HIP_TRY(hipEventRecord(c->sens_ev1, c->stream));
    c->sens_have = true;
    c->sens_plan_kt = kt; c->sens_plan_items = (int)per_img;     // deff_get_plan "sens_kt" / "sens_items": what was launched
    if (g) TRY(rows_d2h(c, g, (const double *)c->sens_g, (size_t)c->rows));
    if (euler) HIP_TRY(hipMemcpyAsync(euler, out, sizeof(double) * c->nimg, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, c->sens_ev0, c->sens_ev1));
    return DEFF_OK;
}

extern "C" int deff_sensitivity_D(deff_ctx *c, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(sens_common(c, "deff_sensitivity_D", CL, CR));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    TRY(ensure_scratch(c, sizeof(double) * c->n));
    double *dD = (double *)c->scratch;
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(dD, 0, sizeof(double) * c->n, c->stream));
    TRY(rows_h2d(c, dD, D, (size_t)c->rows));
    return sens_launch(c, dD, CL, CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_sensitivity(deff_ctx *c, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (c->slab) return fail(DEFF_EINVAL, "deff_sensitivity: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->phase_mode || !c->have_image)
        return fail(DEFF_ESTATE, "deff_sensitivity needs a system assembled from the image (deff_assemble_2phase / _3phase); "
                                 "pass the diffusivities to deff_sensitivity_D() otherwise");
    if (c->native3 || (c->phase_mode == 3 && c->grid_given))
        return fail(DEFF_EINVAL, "deff_sensitivity: the system was assembled with a Grid (identity rows of the flood fill): "
                                 "its Deff is not a function of the phase diffusivities alone");
    TRY(sens_common(c, "deff_sensitivity", c->CL, c->CR));
    TRY(consolidate(c));
    TRY(ensure_scratch(c, sizeof(double) * c->n));
    double *dD = (double *)c->scratch;
    if (c->phase_mode == 2)
        hipLaunchKernelGGL(k_fill_D_2phase, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                           c->nxt, c->ny, c->rows, c->phase_D[0], c->phase_D[1], dD);
    else
        hipLaunchKernelGGL(k_fill_D_3phase, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                           c->nxt, c->ny, c->rows, c->phase_D[0], c->phase_D[1], c->phase_D[2], dD);
    HIP_TRY(hipGetLastError());
    return sens_launch(c, dD, c->CL, c->CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_sensitivity(deff_ctx *c, void **d_g, size_t *row_pitch_bytes)
try {
    if (!c || !d_g) return fail(DEFF_EINVAL, "NULL argument");
    if (!c->sens_have) return fail(DEFF_ESTATE, "no sensitivity map yet (deff_sensitivity / deff_sensitivity_D)");
    *d_g = c->sens_g;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH
