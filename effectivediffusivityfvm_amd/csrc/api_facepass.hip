// api_facepass.hip -- the passes that are one walk over the faces of the current field (kernels_facepass.hpp) and end in one sum
// per image, and the three side vectors they read.  Each pass is one policy of the walk, one __global__ wrapper and one entry
// point below; face_pass_run is the host path of all of them, k_pass_final their final sum.
//   deff_sensitivity / deff_sensitivity_D   SensPass      (x, D) -> dDeff_raw / dD per cell and its Euler sum
//   deff_volume_sensitivity_D               SensPass      on a volume (k_sens3, volume_sens_run; the entry point is in api_volume.hip)
//   deff_field_vjp_D                        VjpPass       (x, lambda, D) -> dL/dD
//   deff_tangent_rhs_D                      TanPass       (x, dD, D) -> r = db - dA x and its squared norm
//   deff_adjoint_tangent_rhs_D              TanPass       on lambda with both wall values 0: q = -dA lambda
//   deff_sensitivity_hvp_D                  HvpPass       (x, dx, dD, D) -> H dD and the curvature dD^T H dD
//   deff_field_vjp_hvp_D                    FieldHvpPass  (x, lambda, dx, dlambda, dD, D) -> S_w dD
// The side vectors (SideVec, ctx.hpp): lambda of A lambda = dL/dx, dx of A dx = r, dlambda of A dlambda = q -- one set, one get
// and one device pointer for the nine entry points; the solves that compute them are in api_cg.hip beside the loop they run.
// A pass reads the field and the vectors; it changes nothing but its own map, its partial sums and the shared upload scratch.
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

// SensPass on a volume: the private context's one tall image of ny rows, slices of sy rows (FpVolume)
__global__ __launch_bounds__(256) void k_sens3(const double *__restrict__ x, const double *__restrict__ D, int nx, int nxt, int ny,
                                               int sy, int ntx, int cpi, int kt, double wx, double wy, double wz, double ww,
                                               double CL, double CR, double den, double *__restrict__ g,
                                               double *__restrict__ partial)
{
    face_pass(SensPass{den}, {x}, D, nx, nxt, ny, 1, ntx, cpi, kt, wx, wy, ww, CL, CR, g, partial, FpVolume{sy, wz});
}

__global__ __launch_bounds__(256) void k_vjp(const double *__restrict__ x, const double *__restrict__ lam,
                                             const double *__restrict__ D, int nx, int nxt, int ny, int nimg, int ntx, int cpi,
                                             int kt, double wx, double wy, double ww, double CL, double CR,
                                             double *__restrict__ g, double *__restrict__ partial)
{
    face_pass(VjpPass{}, {x, lam}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, g, partial);
}

__global__ __launch_bounds__(256) void k_tan(const double *__restrict__ x, const double *__restrict__ dD,
                                             const double *__restrict__ D, int nx, int nxt, int ny, int nimg, int ntx, int cpi,
                                             int kt, double wx, double wy, double ww, double CL, double CR,
                                             double *__restrict__ r, double *__restrict__ partial)
{
    face_pass(TanPass{}, {x, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, r, partial);
}

__global__ __launch_bounds__(256) void k_hvp(const double *__restrict__ x, const double *__restrict__ y,
                                             const double *__restrict__ dD, const double *__restrict__ D, int nx, int nxt, int ny,
                                             int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                             double CR, double den, double *__restrict__ hv, double *__restrict__ partial)
{
    face_pass(HvpPass{den}, {x, y, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, hv, partial);
}

__global__ __launch_bounds__(256) void k_fhvp(const double *__restrict__ x, const double *__restrict__ lam,
                                              const double *__restrict__ y, const double *__restrict__ m,
                                              const double *__restrict__ dD, const double *__restrict__ D, int nx, int nxt, int ny,
                                              int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                              double CR, double *__restrict__ hv, double *__restrict__ partial)
{
    face_pass(FieldHvpPass{}, {x, lam, y, m, dD}, D, nx, nxt, ny, nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, hv, partial);
}

// the final sum of every pass above: an image's partial sums, one workgroup
__global__ __launch_bounds__(1024) void k_pass_final(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    partials_sum_body(partial, per_img, out);
}

}  // namespace deff

// ---- the side vectors ----------------------------------------------------------------------------------------------------

static const char NO_LAMBDA[] = "no adjoint field for the current system (deff_solve_adjoint / deff_set_adjoint)";
static const char NO_DX[] = "no tangent field for the current system (deff_solve_tangent / deff_set_tangent)";
static const char NO_DLAMBDA[] = "no adjoint tangent for the current system and adjoint field (deff_solve_adjoint_tangent / "
                                 "deff_set_adjoint_tangent)";

static int side_vec_need(const deff_ctx *c, SideVec deff_ctx::*which, const char *who, const char *none)
{
    if (!(c->*which).valid) return fail(DEFF_ESTATE, "%s: %s", who, none);
    return DEFF_OK;
}

// A caller's own vector (true width) as `which`.  deff_set_adjoint alone takes one without a system.
static int side_vec_set(deff_ctx *c, SideVec deff_ctx::*which, const char *who, const double *src)
{
    if (!c || !src) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, who));
    const bool lambda = which == &deff_ctx::adj;
    if (!lambda && !c->have_explicit && !c->have_matfree) return fail(DEFF_ESTATE, "no system assembled");
    TRY(use_device(c));
    SideVec &v = c->*which;
    TRY(dev_alloc(&v.x, c->n));
    v.valid = false;
    if (lambda) adjoint_tangent_reset(c);                          // dlambda belonged to the old lambda
    TRY(plane_h2d(c, v.x, src));
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.valid = true;
    return DEFF_OK;
}

static int side_vec_get(deff_ctx *c, SideVec deff_ctx::*which, const char *who, const char *none, double *dst)
{
    if (!c || !dst) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, who));
    TRY(side_vec_need(c, which, who, none));
    TRY(use_device(c));
    TRY(rows_d2h(c, dst, (const double *)(c->*which).x, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}

static int side_vec_device(deff_ctx *c, SideVec deff_ctx::*which, const char *who, const char *none, void **d_v,
                           size_t *row_pitch_bytes)
{
    if (!c || !d_v) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_refused(c, who));
    TRY(side_vec_need(c, which, who, none));
    *d_v = (c->*which).x;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}

extern "C" int deff_set_adjoint(deff_ctx *c, const double *lam)
try { return side_vec_set(c, &deff_ctx::adj, "deff_set_adjoint", lam); }
DEFF_API_CATCH

extern "C" int deff_get_adjoint(deff_ctx *c, double *lam)
try { return side_vec_get(c, &deff_ctx::adj, "deff_get_adjoint", NO_LAMBDA, lam); }
DEFF_API_CATCH

extern "C" int deff_device_adjoint(deff_ctx *c, void **d_lam, size_t *row_pitch_bytes)
try { return side_vec_device(c, &deff_ctx::adj, "deff_device_adjoint", NO_LAMBDA, d_lam, row_pitch_bytes); }
DEFF_API_CATCH

extern "C" int deff_set_tangent(deff_ctx *c, const double *dx)
try { return side_vec_set(c, &deff_ctx::tan, "deff_set_tangent", dx); }
DEFF_API_CATCH

extern "C" int deff_get_tangent(deff_ctx *c, double *dx)
try { return side_vec_get(c, &deff_ctx::tan, "deff_get_tangent", NO_DX, dx); }
DEFF_API_CATCH

extern "C" int deff_device_tangent(deff_ctx *c, void **d_dx, size_t *row_pitch_bytes)
try { return side_vec_device(c, &deff_ctx::tan, "deff_device_tangent", NO_DX, d_dx, row_pitch_bytes); }
DEFF_API_CATCH

extern "C" int deff_set_adjoint_tangent(deff_ctx *c, const double *dl)
try { return side_vec_set(c, &deff_ctx::atan, "deff_set_adjoint_tangent", dl); }
DEFF_API_CATCH

extern "C" int deff_get_adjoint_tangent(deff_ctx *c, double *dl)
try { return side_vec_get(c, &deff_ctx::atan, "deff_get_adjoint_tangent", NO_DLAMBDA, dl); }
DEFF_API_CATCH

extern "C" int deff_device_adjoint_tangent(deff_ctx *c, void **d_dl, size_t *row_pitch_bytes)
try { return side_vec_device(c, &deff_ctx::atan, "deff_device_adjoint_tangent", NO_DLAMBDA, d_dl, row_pitch_bytes); }
DEFF_API_CATCH

// ---- the passes ----------------------------------------------------------------------------------------------------------

// The host path of every pass: the work items of the stack (run length `kt`: the pass's own tuning key), the 2^31 bound, room,
// the timed window, the face weights, `launch(it, wx, wy, ww)` -- the one hipLaunchKernelGGL, on the stack's newest fields
// (x[cur] after consolidate) and planes on the device (pitch nx, pad column 0) --, the final sum and the copies out.
template <typename Launch>
static int face_pass_run(deff_ctx *c, CellPass &p, int kt, const char *who, double *map, double *sums, float *ms, Launch launch)
{
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "%s: too many work items", who);
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, dy = c->dy;
    launch(it, dy / dx, dx / dy, dy / (dx / 2.0));
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_pass_final, it, sums, map, ms);
}

#define FACE_PASS_GRID dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream      /* four waves, one work item each */
#define FACE_PASS_GEOM c->nx, c->nxt, c->ny, c->nimg, it.ntx, it.cpi, it.kt, wx, wy, ww

// D and dD (true width) in the two slots of the upload scratch
static int upload_D_dD(deff_ctx *c, const double *D, const double *dD, const double **d0, const double **d1)
{
    TRY(cell_pass_upload_D(c, D, d0, 0, 2));
    return cell_pass_upload_D(c, dD, d1, 1, 2);
}

// Everything that can refuse the call, before anything is touched.
static int sens_common(deff_ctx *c, const char *who, double CL, double CR)
{
    TRY(slab_refused(c, who));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    if (CR == CL) return fail(DEFF_EINVAL, "%s: CR == CL (Deff is a flux per unit of CR - CL)", who);
    TRY(use_device(c));
    return DEFF_OK;
}

static int sens_run(deff_ctx *c, const double *dD, double CL, double CR, double *g, double *euler, float *ms)
{
    const double den = (CR - CL) * (CR - CL);
    return face_pass_run(c, c->pass_sens, c->pass_sens.kt, "deff_sensitivity", g, euler, ms,
                         [=](const CellItems &it, double wx, double wy, double ww) {
                             hipLaunchKernelGGL(k_sens, FACE_PASS_GRID, c->x[c->cur], dD, FACE_PASS_GEOM, CL, CR, den,
                                                c->pass_sens.map, c->pass_sens.part);
                         });
}

extern "C" int deff_sensitivity_D(deff_ctx *c, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(sens_common(c, "deff_sensitivity_D", CL, CR));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    return sens_run(c, dD, CL, CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_sensitivity(deff_ctx *c, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    TRY(slab_refused(c, "deff_sensitivity"));
    const double *dD;
    TRY(image_D_plane(c, "deff_sensitivity", "its Deff is", [c] {
        TRY(sens_common(c, "deff_sensitivity", c->CL, c->CR));
        return consolidate(c);
    }, &dD));
    return sens_run(c, dD, c->CL, c->CR, g, euler, ms);
}
DEFF_API_CATCH

// deff_volume_sensitivity_D (api_volume.hip) on the volume's private context c of nx x (ny * nz), one image: face_pass_run's
// steps with the volume's own face weights (c->dy is not the volume's and is not read) and k_sens3.  The caller has refused
// what can be refused.
int volume_sens_run(deff_ctx *c, const double *D, int ny, double dy, double dz, double CL, double CR, double *g, double *euler,
                    float *ms)
{
    TRY(use_device(c));
    TRY(consolidate(c));
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    CellPass &p = c->pass_sens;
    const CellItems it = cell_pass_items(c->nxt, c->ny, 1, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_volume_sensitivity_D: too many work items");
    TRY(cell_pass_room(c, p, true, it.items));
    TRY(cell_pass_start(c, p, ms));
    const double dx = c->dx, den = (CR - CL) * (CR - CL);
    hipLaunchKernelGGL(k_sens3, FACE_PASS_GRID, c->x[c->cur], dD, c->nx, c->nxt, c->ny, ny, it.ntx, it.cpi, it.kt, dy * dz / dx,
                       dx * dz / dy, dx * dy / dz, dy * dz / (dx / 2.0), CL, CR, den, p.map, p.part);
    HIP_TRY(hipGetLastError());
    return cell_pass_finish(c, p, k_pass_final, it, euler, g, ms);
}

extern "C" int deff_field_vjp_D(deff_ctx *c, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(slab_refused(c, "deff_field_vjp_D"));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(side_vec_need(c, &deff_ctx::adj, "deff_field_vjp_D", NO_LAMBDA));
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    return face_pass_run(c, c->pass_vjp, c->pass_vjp.kt, "deff_field_vjp_D", g, euler, ms,
                         [=](const CellItems &it, double wx, double wy, double ww) {
                             hipLaunchKernelGGL(k_vjp, FACE_PASS_GRID, c->x[c->cur], c->adj.x, dD, FACE_PASS_GEOM, CL, CR,
                                                c->pass_vjp.map, c->pass_vjp.part);
                         });
}
DEFF_API_CATCH

// k_tan on `field` -- the stack's newest fields into pass_tan, or lambda into pass_atan -- for the planes d0 = D and d1 = dD; both
// passes are planned by tuning "tan_kt"
static int tan_run(deff_ctx *c, CellPass &p, const char *who, const double *field, const double *d0, const double *d1, double CL,
                   double CR, double *r, double *norm2, float *ms)
{
    return face_pass_run(c, p, c->pass_tan.kt, who, r, norm2, ms, [=, &p](const CellItems &it, double wx, double wy, double ww) {
        hipLaunchKernelGGL(k_tan, FACE_PASS_GRID, field, d1, d0, FACE_PASS_GEOM, CL, CR, p.map, p.part);
    });
}

extern "C" int deff_tangent_rhs_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *r, double *norm2,
                                  float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    TRY(slab_refused(c, "deff_tangent_rhs_D"));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(upload_D_dD(c, D, dD, &d0, &d1));
    TRY(tan_run(c, c->pass_tan, "deff_tangent_rhs_D", c->x[c->cur], d0, d1, CL, CR, r, norm2, ms));
    c->tan.rhs_ok = true;                                          // a right-hand side for the current system
    return DEFF_OK;
}
DEFF_API_CATCH

// The right-hand side of lambda's own tangent (the second-order field adjoint): differentiating A lambda = w along dD with w
// fixed, A dlambda = -dA lambda =: q -- the pass above with lambda in the place of the field and both wall values 0 (db is the
// walls' part: lambda has none).  Into pass_atan: pass_tan's map, which deff_solve_tangent reads, stays.
extern "C" int deff_adjoint_tangent_rhs_D(deff_ctx *c, const double *D, const double *dD, double *q, double *norm2, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    TRY(slab_refused(c, "deff_adjoint_tangent_rhs_D"));
    TRY(side_vec_need(c, &deff_ctx::adj, "deff_adjoint_tangent_rhs_D", NO_LAMBDA));
    TRY(use_device(c));
    TRY(resident_check(c));                                        // the scratch and the stream are about to be used
    const double *d0, *d1;
    TRY(upload_D_dD(c, D, dD, &d0, &d1));
    TRY(tan_run(c, c->pass_atan, "deff_adjoint_tangent_rhs_D", c->adj.x, d0, d1, 0.0, 0.0, q, norm2, ms));
    c->atan.rhs_ok = true;                                         // a right-hand side for the current system and lambda
    c->atan.valid = false;                                         // dlambda belonged to the previous one
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_sensitivity_hvp_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *hv,
                                      double *curv, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    TRY(slab_refused(c, "deff_sensitivity_hvp_D"));
    if (CR == CL) return fail(DEFF_EINVAL, "deff_sensitivity_hvp_D: CR == CL (Deff is a flux per unit of CR - CL)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(side_vec_need(c, &deff_ctx::tan, "deff_sensitivity_hvp_D", NO_DX));
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(upload_D_dD(c, D, dD, &d0, &d1));
    const double den = (CR - CL) * (CR - CL);
    return face_pass_run(c, c->pass_hvp, c->pass_hvp.kt, "deff_sensitivity_hvp_D", hv, curv, ms,
                         [=](const CellItems &it, double wx, double wy, double ww) {
                             hipLaunchKernelGGL(k_hvp, FACE_PASS_GRID, c->x[c->cur], c->tan.x, d1, d0, FACE_PASS_GEOM, CL, CR, den,
                                                c->pass_hvp.map, c->pass_hvp.part);
                         });
}
DEFF_API_CATCH

extern "C" int deff_field_vjp_hvp_D(deff_ctx *c, const double *D, const double *dD, double CL, double CR, double *hv,
                                    double *curv, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!dD) return fail(DEFF_EINVAL, "dD is NULL");
    TRY(slab_refused(c, "deff_field_vjp_hvp_D"));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(side_vec_need(c, &deff_ctx::adj, "deff_field_vjp_hvp_D", NO_LAMBDA));
    TRY(side_vec_need(c, &deff_ctx::tan, "deff_field_vjp_hvp_D", NO_DX));
    TRY(side_vec_need(c, &deff_ctx::atan, "deff_field_vjp_hvp_D", NO_DLAMBDA));
    TRY(use_device(c));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *d0, *d1;
    TRY(upload_D_dD(c, D, dD, &d0, &d1));
    return face_pass_run(c, c->pass_fhvp, c->pass_fhvp.kt, "deff_field_vjp_hvp_D", hv, curv, ms,
                         [=](const CellItems &it, double wx, double wy, double ww) {
                             hipLaunchKernelGGL(k_fhvp, FACE_PASS_GRID, c->x[c->cur], c->adj.x, c->tan.x, c->atan.x, d1, d0,
                                                FACE_PASS_GEOM, CL, CR, c->pass_fhvp.map, c->pass_fhvp.part);
                         });
}
DEFF_API_CATCH

// ---- the last map of each pass, on the device ----------------------------------------------------------------------------

extern "C" int deff_device_sensitivity(deff_ctx *c, void **d_map, size_t *row_pitch_bytes)
try { return cell_pass_device_map(c, &deff_ctx::pass_sens, d_map, row_pitch_bytes, "no sensitivity map yet (deff_sensitivity / deff_sensitivity_D)"); }
DEFF_API_CATCH

extern "C" int deff_device_field_vjp(deff_ctx *c, void **d_map, size_t *row_pitch_bytes)
try { return cell_pass_device_map(c, &deff_ctx::pass_vjp, d_map, row_pitch_bytes, "no field-adjoint map yet (deff_field_vjp_D)"); }
DEFF_API_CATCH

extern "C" int deff_device_tangent_rhs(deff_ctx *c, void **d_map, size_t *row_pitch_bytes)
try { return cell_pass_device_map(c, &deff_ctx::pass_tan, d_map, row_pitch_bytes, "no tangent right-hand side yet (deff_tangent_rhs_D)"); }
DEFF_API_CATCH

extern "C" int deff_device_sensitivity_hvp(deff_ctx *c, void **d_map, size_t *row_pitch_bytes)
try { return cell_pass_device_map(c, &deff_ctx::pass_hvp, d_map, row_pitch_bytes, "no Hessian-vector map yet (deff_sensitivity_hvp_D)"); }
DEFF_API_CATCH

extern "C" int deff_device_field_vjp_hvp(deff_ctx *c, void **d_map, size_t *row_pitch_bytes)
try { return cell_pass_device_map(c, &deff_ctx::pass_fhvp, d_map, row_pitch_bytes, "no second-order field-adjoint map yet (deff_field_vjp_hvp_D)"); }
DEFF_API_CATCH
