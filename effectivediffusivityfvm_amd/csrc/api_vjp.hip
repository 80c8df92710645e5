// api_vjp.hip -- the field adjoint's buffer and pass: deff_set_adjoint / deff_get_adjoint / deff_device_adjoint (lambda of
// A lambda = dL/dx; deff_solve_adjoint, which computes it, is in api_cg.hip beside the loop it runs) and deff_field_vjp_D /
// deff_device_field_vjp: g = dL/dD per cell and its Euler sum from the current field, lambda and D, one pass on the device
// (kernels_vjp.hpp).  Reads the field and lambda; changes nothing but the map, its partial sums and the shared upload scratch.
#include "ctx.hpp"
#include "kernels_vjp.hpp"
#include <algorithm>

extern "C" int deff_set_adjoint(deff_ctx *c, const double *lam)
try {
    if (!c || !lam) return fail(DEFF_EINVAL, "NULL argument");
    if (c->slab) return fail(DEFF_EINVAL, "deff_set_adjoint: not for row-slab contexts (the rows of the image live on several devices)");
    TRY(use_device(c));
    TRY(dev_alloc(&c->adj_lam, c->n));
    c->adj_valid = false;
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
    // work items as the gradient pass's (api_sens.hip): column strips of 128, cut into runs of kt tiles of VJP_ROWS rows, about
    // 4 096 items in a launch and at most 16 384 per image; tuning "vjp_kt" overrides
    const int ntx = (c->nxt + VJP_COLS - 1) / VJP_COLS, tiles_y = (c->ny + VJP_ROWS - 1) / VJP_ROWS;
    int kt = c->vjp_kt;
    if (kt <= 0) {
        kt = (int)std::min<size_t>(64, std::max<size_t>(1, (size_t)ntx * tiles_y * c->nimg / 4096));
        kt = std::max(kt, (int)(((size_t)ntx * tiles_y + 16383) / 16384));
    }
    if (kt > tiles_y) kt = tiles_y;
    const int cpi = (tiles_y + kt - 1) / kt;
    const size_t per_img = (size_t)ntx * cpi, items = per_img * c->nimg;
    if ((items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_field_vjp_D: too many work items");
    TRY(dev_alloc(&c->vjp_g, c->n));
    const size_t want = items + (size_t)c->nimg;
    if (c->vjp_part_cap < want) {
        if (c->vjp_part) { HIP_TRY(hipFree(c->vjp_part)); c->vjp_part = nullptr; c->vjp_part_cap = 0; }
        HIP_TRY(hipMalloc((void **)&c->vjp_part, want * sizeof(double)));
        c->vjp_part_cap = want;
    }
    if (ms) {                                                      // the call's own pair: ev0 / ev1 belong to the solve loops
        if (!c->vjp_ev0) HIP_TRY(hipEventCreate(&c->vjp_ev0));
        if (!c->vjp_ev1) HIP_TRY(hipEventCreate(&c->vjp_ev1));
        HIP_TRY(hipEventRecord(c->vjp_ev0, c->stream));
    }
    const double dx = c->dx, dy = c->dy;
    const double wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0);
    double *out = c->vjp_part + items;
    hipLaunchKernelGGL(k_vjp, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], c->adj_lam, dD, c->nx,
                       c->nxt, c->ny, c->nimg, ntx, cpi, kt, wx, wy, ww, CL, CR, c->vjp_g, c->vjp_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vjp_final, dim3(c->nimg), dim3(1024), 0, c->stream, c->vjp_part, per_img, out);
    HIP_TRY(hipGetLastError());
    if (ms) HIP_TRY(hipEventRecord(c->vjp_ev1, c->stream));
    c->vjp_have = true;
    c->vjp_plan_kt = kt; c->vjp_plan_items = (int)per_img;       // deff_get_plan "vjp_kt" / "vjp_items": what was launched
    if (g) TRY(rows_d2h(c, g, (const double *)c->vjp_g, (size_t)c->rows));
    if (euler) HIP_TRY(hipMemcpyAsync(euler, out, sizeof(double) * c->nimg, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, c->vjp_ev0, c->vjp_ev1));
    return DEFF_OK;
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
    TRY(ensure_scratch(c, sizeof(double) * c->n));
    double *dD = (double *)c->scratch;
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(dD, 0, sizeof(double) * c->n, c->stream));
    TRY(rows_h2d(c, dD, D, (size_t)c->rows));
    return vjp_launch(c, dD, CL, CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_field_vjp(deff_ctx *c, void **d_g, size_t *row_pitch_bytes)
try {
    if (!c || !d_g) return fail(DEFF_EINVAL, "NULL argument");
    if (!c->vjp_have) return fail(DEFF_ESTATE, "no field-adjoint map yet (deff_field_vjp_D)");
    *d_g = c->vjp_g;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH
