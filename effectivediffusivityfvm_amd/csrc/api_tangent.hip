// api_tangent.hip -- the field tangent's pass and buffer: deff_tangent_rhs_D / deff_device_tangent_rhs: r = db - dA x per cell
// for a direction dD and its squared norm per image, from the current field, D and dD, one pass on the device
// (kernels_facepass.hpp: the walk with TanPass); deff_get_tangent / deff_device_tangent: dx of A dx = r' (deff_solve_tangent,
// which computes it, is in api_cg.hip beside the loop it runs); deff_adjoint_tangent_rhs_D: the same pass on lambda, the
// right-hand side of the adjoint's tangent (api_fhvp.hip).  Reads the field (lambda); changes nothing but the map, its partial
// sums and the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_facepass.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the face walk's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_tan(const double *__restrict__ x, const double *__restrict__ dD,
                                             const double *__restrict__ D, int nx, int nxt, int ny, int nimg, int ntx, int cpi,
                                             int kt, double wx, double wy, double ww, double CL, double CR,
                                             double *__restrict__ r, double *__restrict__ partial)
{
    face_pass(TanPass{}, {x, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, r, partial);
}

__global__ __launch_bounds__(1024) void k_tan_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

// the map of `field` -- the stack's newest fields (x[cur] after consolidate) into pass_tan, or lambda into pass_atan -- for the
// planes `dD` and `ddD` on the device (pitch nx, pad column 0); both passes are planned by tuning "tan_kt"
static int tan_launch(deff_ctx *c, CellPass &p, const char *who, const double *field, const double *dD, const double *ddD, double CL,
                      double CR, double *r, double *norm2, float *ms)
{
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, c->pass_tan.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "%s: too many work items", who);
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0);
    hipLaunchKernelGGL(k_tan, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, field, ddD, dD, c->nx, c->nxt,
                       c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww, CL, CR, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_tan_final, it, norm2, r, ms);
}

extern "C" int deff_tangent_rhs_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *r, double *norm2,
                                  float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    if (c->slab) return fail(DEFF_EINVAL, "deff_tangent_rhs_D: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(cell_pass_upload_D(c, D, &d0, 0, 2));
    TRY(cell_pass_upload_D(c, dD, &d1, 1, 2));
    TRY(tan_launch(c, c->pass_tan, "deff_tangent_rhs_D", c->x[c->cur], d0, d1, CL, CR, r, norm2, ms));
    c->tan_rhs = true;                                             // a right-hand side for the current system
    return DEFF_OK;
}
DEFF_API_CATCH

// The right-hand side of lambda's own tangent (the second-order field adjoint, api_fhvp.hip): differentiating A lambda = w along
// dD with w fixed, A dlambda = -dA lambda =: q -- the pass above with lambda in the place of the field and both wall values 0
// (db is the walls' part: lambda has none).  Into pass_atan: pass_tan's map, which deff_solve_tangent reads, stays.
extern "C" int deff_adjoint_tangent_rhs_D(deff_ctx *c, const double *D, const double *dD, double *q, double *norm2, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    if (c->slab)
        return fail(DEFF_EINVAL, "deff_adjoint_tangent_rhs_D: not for row-slab contexts (the rows of the image live on several devices)");
    if (!c->adj_valid)
        return fail(DEFF_ESTATE, "deff_adjoint_tangent_rhs_D: no adjoint field for the current system (deff_solve_adjoint / deff_set_adjoint)");
    TRY(use_device(c));
    TRY(resident_check(c));                                        // the scratch and the stream are about to be used
    const double *d0, *d1;
    TRY(cell_pass_upload_D(c, D, &d0, 0, 2));
    TRY(cell_pass_upload_D(c, dD, &d1, 1, 2));
    TRY(tan_launch(c, c->pass_atan, "deff_adjoint_tangent_rhs_D", c->adj_lam, d0, d1, 0.0, 0.0, q, norm2, ms));
    c->atan_rhs = true;                                            // a right-hand side for the current system and lambda
    c->atan_valid = false;                                         // dlambda belonged to the previous one
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_device_tangent_rhs(deff_ctx *c, void **d_r, size_t *row_pitch_bytes)
try {
    return cell_pass_device_map(c, &deff_ctx::pass_tan, d_r, row_pitch_bytes, "no tangent right-hand side yet (deff_tangent_rhs_D)");
}
DEFF_API_CATCH

static int tangent_common(deff_ctx *c, const char *who)
{
    if (c->slab) return fail(DEFF_EINVAL, "%s: not for row-slab contexts (the rows of the image live on several devices)", who);
    if (!c->tan_valid) return fail(DEFF_ESTATE, "%s: no tangent field for the current system (deff_solve_tangent / deff_set_tangent)", who);
    return DEFF_OK;
}

extern "C" int deff_get_tangent(deff_ctx *c, double *dx)
try {
    if (!c || !dx) return fail(DEFF_EINVAL, "NULL argument");
    TRY(tangent_common(c, "deff_get_tangent"));
    TRY(use_device(c));
    TRY(rows_d2h(c, dx, (const double *)c->tan_dx, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_device_tangent(deff_ctx *c, void **d_dx, size_t *row_pitch_bytes)
try {
    if (!c || !d_dx) return fail(DEFF_EINVAL, "NULL argument");
    TRY(tangent_common(c, "deff_device_tangent"));
    *d_dx = c->tan_dx;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH
