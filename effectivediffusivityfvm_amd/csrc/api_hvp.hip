// api_hvp.hip -- the Deff Hessian-vector product's pass: deff_sensitivity_hvp_D / deff_device_sensitivity_hvp: hv = H dD per
// cell, H the Hessian of Deff_raw with respect to the diffusivity map, and the curvature dD^T H dD per image, from the current
// field, the current tangent dx (deff_solve_tangent along the same dD, or deff_set_tangent), D and dD, one pass on the device
// (kernels_facepass.hpp: the walk with HvpPass); and deff_set_tangent, a caller's own dx.  The pass reads the field and dx;
// it changes nothing but the map, its partial sums and the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_facepass.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the face walk's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_hvp(const double *__restrict__ x, const double *__restrict__ y,
                                             const double *__restrict__ dD, const double *__restrict__ D, int nx, int nxt, int ny,
                                             int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                             double CR, double den, double *__restrict__ hv, double *__restrict__ partial)
{
    face_pass(HvpPass{den}, {x, y, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, hv, partial);
}

__global__ __launch_bounds__(1024) void k_hvp_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

extern "C" int deff_set_tangent(deff_ctx *c, const double *dx)
try {
    if (!c || !dx) return fail(DEFF_EINVAL, "NULL argument");
    if (c->slab) return fail(DEFF_EINVAL, "deff_set_tangent: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->have_explicit && !c->have_matfree) return fail(DEFF_ESTATE, "no system assembled");
    TRY(use_device(c));
    TRY(dev_alloc(&c->tan_dx, c->n));
    c->tan_valid = false;
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(c->tan_dx, 0, sizeof(double) * c->n, c->stream));
    TRY(rows_h2d(c, c->tan_dx, dx, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tan_valid = true;
    return DEFF_OK;
}
DEFF_API_CATCH

// the map of the stack's newest fields (x[cur] after consolidate) and dx for the planes `dD` and `ddD` on the device (pitch nx, pad column 0)
static int hvp_launch(deff_ctx *c, const double *dD, const double *ddD, double CL, double CR, double *hv, double *curv, float *ms)
{
    CellPass &p = c->pass_hvp;
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_sensitivity_hvp_D: too many work items");
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), den = (CR - CL) * (CR - CL);
    hipLaunchKernelGGL(k_hvp, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], c->tan_dx, ddD, dD,
                       c->nx, c->nxt, c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww, CL, CR, den, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_hvp_final, it, curv, hv, ms);
}

extern "C" int deff_sensitivity_hvp_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *hv,
                                      double *curv, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    if (c->slab)
        return fail(DEFF_EINVAL, "deff_sensitivity_hvp_D: not for row-slab contexts (the rows of the image live on several devices)");
    if (CR == CL) return fail(DEFF_EINVAL, "deff_sensitivity_hvp_D: CR == CL (Deff is a flux per unit of CR - CL)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    if (!c->tan_valid)
        return fail(DEFF_ESTATE, "deff_sensitivity_hvp_D: no tangent field for the current system (deff_solve_tangent / deff_set_tangent)");
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(cell_pass_upload_D(c, D, &d0, 0, 2));
    TRY(cell_pass_upload_D(c, dD, &d1, 1, 2));
    return hvp_launch(c, d0, d1, CL, CR, hv, curv, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_sensitivity_hvp(deff_ctx *c, void **d_hv, size_t *row_pitch_bytes)
try {
    return cell_pass_device_map(c, &deff_ctx::pass_hvp, d_hv, row_pitch_bytes,
                                "no Hessian-vector map yet (deff_sensitivity_hvp_D)");
}
DEFF_API_CATCH
