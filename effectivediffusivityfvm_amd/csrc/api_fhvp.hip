// api_fhvp.hip -- the field adjoint's second order: hv = S_w dD per cell, S_w the Hessian of w^T x(D) with w = dL/dx fixed.
// deff_get_adjoint_tangent / deff_device_adjoint_tangent / deff_set_adjoint_tangent: dlambda of A dlambda = q = -dA lambda
// (deff_adjoint_tangent_rhs_D, which computes q with k_tan, is in api_tangent.hip beside that kernel; deff_solve_adjoint_tangent
// is in api_cg.hip beside the loop it runs); deff_field_vjp_hvp_D / deff_device_field_vjp_hvp: the pass over
// (x, lambda, dx, dlambda, dD, D) and dD^T S_w dD per image (kernels_facepass.hpp: the walk with FieldHvpPass).  The passes
// read the field, lambda, dx and dlambda; they change nothing but their own map, its partial sums and the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_facepass.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the face walk's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_fhvp(const double *__restrict__ x, const double *__restrict__ lam,
                                              const double *__restrict__ y, const double *__restrict__ m,
                                              const double *__restrict__ dD, const double *__restrict__ D, int nx, int nxt, int ny,
                                              int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                              double CR, double *__restrict__ hv, double *__restrict__ partial)
{
    face_pass(FieldHvpPass{}, {x, lam, y, m, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, hv, partial);
}

__global__ __launch_bounds__(1024) void k_fhvp_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

static int slab_refused(deff_ctx *c, const char *who)
{
    if (c->slab) return fail(DEFF_EINVAL, "%s: not for row-slab contexts (the rows of the image live on several devices)", who);
    return DEFF_OK;
}

static int need_adjoint(deff_ctx *c, const char *who)
{
    if (!c->adj_valid)
        return fail(DEFF_ESTATE, "%s: no adjoint field for the current system (deff_solve_adjoint / deff_set_adjoint)", who);
    return DEFF_OK;
}

static int need_adjoint_tangent(deff_ctx *c, const char *who)
{
    if (!c->atan_valid)
        return fail(DEFF_ESTATE, "%s: no adjoint tangent for the current system and adjoint field (deff_solve_adjoint_tangent / "
                                 "deff_set_adjoint_tangent)", who);
    return DEFF_OK;
}

extern "C" int deff_set_adjoint_tangent(deff_ctx *c, const double *dl)
try {
    if (!c || !dl) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, "deff_set_adjoint_tangent"));
    if (!c->have_explicit && !c->have_matfree) return fail(DEFF_ESTATE, "no system assembled");
    TRY(use_device(c));
    TRY(dev_alloc(&c->adj_dl, c->n));
    c->atan_valid = false;
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(c->adj_dl, 0, sizeof(double) * c->n, c->stream));
    TRY(rows_h2d(c, c->adj_dl, dl, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->atan_valid = true;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_get_adjoint_tangent(deff_ctx *c, double *dl)
try {
    if (!c || !dl) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, "deff_get_adjoint_tangent"));
    TRY(need_adjoint_tangent(c, "deff_get_adjoint_tangent"));
    TRY(use_device(c));
    TRY(rows_d2h(c, dl, (const double *)c->adj_dl, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_device_adjoint_tangent(deff_ctx *c, void **d_dl, size_t *row_pitch_bytes)
try {
    if (!c || !d_dl) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, "deff_device_adjoint_tangent"));
    TRY(need_adjoint_tangent(c, "deff_device_adjoint_tangent"));
    *d_dl = c->adj_dl;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH

// the map of the stack's newest fields (x[cur] after consolidate), lambda, dx and dlambda for the planes `dD` and `ddD` on the
// device (pitch nx, pad column 0)
static int fhvp_launch(deff_ctx *c, const double *dD, const double *ddD, double CL, double CR, double *hv, double *curv, float *ms)
{
    CellPass &p = c->pass_fhvp;
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_field_vjp_hvp_D: too many work items");
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0);
    hipLaunchKernelGGL(k_fhvp, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], c->adj_lam, c->tan_dx,
                       c->adj_dl, ddD, dD, c->nx, c->nxt, c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww, CL, CR, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_fhvp_final, it, curv, hv, ms);
}

extern "C" int deff_field_vjp_hvp_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *hv,
                                    double *curv, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    TRY(slab_refused(c, "deff_field_vjp_hvp_D"));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(need_adjoint(c, "deff_field_vjp_hvp_D"));
    if (!c->tan_valid)
        return fail(DEFF_ESTATE, "deff_field_vjp_hvp_D: no tangent field for the current system (deff_solve_tangent / deff_set_tangent)");
    TRY(need_adjoint_tangent(c, "deff_field_vjp_hvp_D"));
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(cell_pass_upload_D(c, D, &d0, 0, 2));
    TRY(cell_pass_upload_D(c, dD, &d1, 1, 2));
    return fhvp_launch(c, d0, d1, CL, CR, hv, curv, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_field_vjp_hvp(deff_ctx *c, void **d_hv, size_t *row_pitch_bytes)
try {
    return cell_pass_device_map(c, &deff_ctx::pass_fhvp, d_hv, row_pitch_bytes,
                                "no second-order field-adjoint map yet (deff_field_vjp_hvp_D)");
}
DEFF_API_CATCH
