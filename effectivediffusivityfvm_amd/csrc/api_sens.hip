// api_sens.hip -- deff_sensitivity / deff_sensitivity_D / deff_device_sensitivity: the per-cell gradient dDeff_raw / dD of the
// context's current field and its Euler sum, one pass on the device (kernels_facepass.hpp: the walk with SensPass).  Reads the
// field; changes nothing but the map, its partial sums and the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_facepass.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the face walk's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_sens(const double *__restrict__ x, const double *__restrict__ D, int nx, int nxt, int ny,
                                              int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                              double CR, double den, double *__restrict__ g, double *__restrict__ partial)
{
    face_pass(SensPass{den}, {x}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, g, partial);
}

__global__ __launch_bounds__(1024) void k_sens_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

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
    CellPass &p = c->pass_sens;
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_sensitivity: too many work items");
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), den = (CR - CL) * (CR - CL);
    hipLaunchKernelGGL(k_sens, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], dD, c->nx, c->nxt,
                       c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww, CL, CR, den, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_sens_final, it, euler, g, ms);
}

extern "C" int deff_sensitivity_D(deff_ctx *c, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(sens_common(c, "deff_sensitivity_D", CL, CR));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
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
    return cell_pass_device_map(c, &deff_ctx::pass_sens, d_g, row_pitch_bytes,
                                "no sensitivity map yet (deff_sensitivity / deff_sensitivity_D)");
}
DEFF_API_CATCH
