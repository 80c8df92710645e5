// api_vjp.hip -- the field adjoint's buffer and pass: deff_set_adjoint / deff_get_adjoint / deff_device_adjoint (lambda of
// A lambda = dL/dx; deff_solve_adjoint, which computes it, is in api_cg.hip beside the loop it runs) and deff_field_vjp_D /
// deff_device_field_vjp: g = dL/dD per cell and its Euler sum from the current field, lambda and D, one pass on the device
// (kernels_facepass.hpp: the walk with VjpPass).  Reads the field and lambda; changes nothing but the map, its partial sums and
// the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_facepass.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the face walk's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_vjp(const double *__restrict__ x, const double *__restrict__ lam,
                                             const double *__restrict__ D, int nx, int nxt, int ny, int nimg, int ntx, int cpi,
                                             int kt, double wx, double wy, double ww, double CL, double CR,
                                             double *__restrict__ g, double *__restrict__ partial)
{
    face_pass(VjpPass{}, {x, lam}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, g, partial);
}

__global__ __launch_bounds__(1024) void k_vjp_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

extern "C" int deff_set_adjoint(deff_ctx *c, const double *lam)
try {
    if (!c || !lam) return fail(DEFF_EINVAL, "NULL argument");
    if (c->slab) return fail(DEFF_EINVAL, "deff_set_adjoint: not for row-slab contexts (the rows of the image live on several devices)");
    TRY(use_device(c));
    TRY(dev_alloc(&c->adj_lam, c->n));
    c->adj_valid = false;
    adjoint_tangent_reset(c);                                      // dlambda (api_fhvp.hip) belonged to the old lambda
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(c->adj_lam, 0, sizeof(double) * c->n, c->stream));
    TRY(rows_h2d(c, c->adj_lam, lam, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->adj_valid = true;
    return DEFF_OK;
}
DEFF_API_CATCH

static int adjoint_common(deff_ctx *c, const char *who)
{
    if (c->slab) return fail(DEFF_EINVAL, "%s: not for row-slab contexts (the rows of the image live on several devices)", who);
    if (!c->adj_valid)
        return fail(DEFF_ESTATE, "%s: no adjoint field for the current system (deff_solve_adjoint / deff_set_adjoint)", who);
    return DEFF_OK;
}

extern "C" int deff_get_adjoint(deff_ctx *c, double *lam)
try {
    if (!c || !lam) return fail(DEFF_EINVAL, "NULL argument");
    TRY(adjoint_common(c, "deff_get_adjoint"));
    TRY(use_device(c));
    TRY(rows_d2h(c, lam, (const double *)c->adj_lam, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_device_adjoint(deff_ctx *c, void **d_lam, size_t *row_pitch_bytes)
try {
    if (!c || !d_lam) return fail(DEFF_EINVAL, "NULL argument");
    TRY(adjoint_common(c, "deff_device_adjoint"));
    *d_lam = c->adj_lam;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH

// the map of the stack's newest fields (x[cur] after consolidate) and lambda for the D plane `dD` on the device (pitch nx, pad column 0)
static int vjp_launch(deff_ctx *c, const double *dD, double CL, double CR, double *g, double *euler, float *ms)
{
    CellPass &p = c->pass_vjp;
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_field_vjp_D: too many work items");
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0);
    hipLaunchKernelGGL(k_vjp, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], c->adj_lam, dD, c->nx,
                       c->nxt, c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww, CL, CR, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_vjp_final, it, euler, g, ms);
}

extern "C" int deff_field_vjp_D(deff_ctx *c, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (c->slab) return fail(DEFF_EINVAL, "deff_field_vjp_D: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(adjoint_common(c, "deff_field_vjp_D"));
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    return vjp_launch(c, dD, CL, CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_field_vjp(deff_ctx *c, void **d_g, size_t *row_pitch_bytes)
try {
    return cell_pass_device_map(c, &deff_ctx::pass_vjp, d_g, row_pitch_bytes, "no field-adjoint map yet (deff_field_vjp_D)");
}
DEFF_API_CATCH
