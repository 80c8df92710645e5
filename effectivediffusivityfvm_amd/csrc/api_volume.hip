// api_volume.hip -- 3-D volumes (include/deff_amd.h, "volumes"): a host D volume in, a field converged to
// ||b - A x|| <= rtol ||b|| and its Deff out.  A deff_volume owns a private deff_ctx of nx x (ny * nz), one image -- slice k is
// rows [k * ny, (k + 1) * ny) of it -- plus the planes aB and aF that couple row l to rows l - ny and l + ny.  The field, the
// linear guess, the wall fluxes and Deff (the mean wall flux density over all ny * nz rows) are the context's own; the
// assembly, the admissibility pass and the iteration are the volume's kernels (kernels_cg_volume.hpp, launched from
// api_cg.hip).  A type of its own because every 2-D entry point would be wrong on a volume: it cannot be passed to them.
#include "ctx.hpp"

struct deff_volume {
    deff_ctx *c = nullptr;          // nx x (ny * nz); its dy is not the volume's and is never read
    int ny = 0, nz = 0;
    double dy = 0, dz = 0;
    double *aB = nullptr, *aF = nullptr;         // device, pitch c->nx
    bool have_system = false;
};

extern "C" int deff_volume_destroy(deff_volume *v)
try {
    if (!v) return DEFF_OK;
    if (v->c) {
        (void)hipSetDevice(v->c->device);
        if (v->c->stream) (void)hipStreamSynchronize(v->c->stream);
    }
    if (v->aB) (void)hipFree(v->aB);
    if (v->aF) (void)hipFree(v->aF);
    const int rc = deff_destroy(v->c);
    delete v;
    return rc;
}
DEFF_API_CATCH

extern "C" int deff_volume_create(int device, int nx, int ny, int nz, deff_volume **out)
try {
    if (!out) return fail(DEFF_EINVAL, "out is NULL");
    *out = nullptr;
    if (nx < 2 || ny < 2 || nz < 1) return fail(DEFF_EINVAL, "a volume must be at least 2x2x1 (got %dx%dx%d)", nx, ny, nz);
    if ((long long)ny * nz > (1ll << 30)) return fail(DEFF_EINVAL, "a volume of %dx%dx%d exceeds 2^31 cells", nx, ny, nz);
    deff_volume *v = new (std::nothrow) deff_volume();
    if (!v) return fail(DEFF_ENOMEM, "host allocation failed");
    struct Guard { deff_volume *v; ~Guard() { if (v) deff_volume_destroy(v); } } guard{v};   // until handed to the caller
    TRY(deff_create(device, nx, ny * nz, &v->c));
    v->ny = ny;
    v->nz = nz;
    v->dy = 1.0 / ny;               // the unit cube
    v->dz = 1.0 / nz;
    TRY(dev_alloc(&v->aB, v->c->n));
    TRY(dev_alloc(&v->aF, v->c->n));
    guard.v = nullptr;
    *out = v;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_volume_mesh(const deff_volume *v, int *nx, int *ny, int *nz, double *dx, double *dy, double *dz)
try {
    if (!v) return fail(DEFF_EINVAL, "volume is NULL");
    if (nx) *nx = v->c->nxt;
    if (ny) *ny = v->ny;
    if (nz) *nz = v->nz;
    if (dx) *dx = v->c->dx;
    if (dy) *dy = v->dy;
    if (dz) *dz = v->dz;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_volume_assemble_from_D(deff_volume *v, const double *D, double CL, double CR)
try {
    if (!v || !D) return fail(DEFF_EINVAL, "NULL argument");
    deff_ctx *c = v->c;
    TRY(use_device(c));
    TRY(ensure_explicit(c));
    TRY(ensure_walls(c));
    const size_t bytes = sizeof(double) * c->n;
    TRY(ensure_scratch(c, bytes));
    double *dD = (double *)c->scratch;
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(c->scratch, 0, bytes, c->stream));
    TRY(rows_h2d(c, dD, D, (size_t)c->rows));
    c->CL = CL; c->CR = CR;
    TRY(volume_assemble_planes(c, dD, v->ny, v->nz, v->dy, v->dz, CL, CR, v->aB, v->aF));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the private context holds planes that no 2-D path may take for a 2-D system's: it is reachable through the volume's
    // entry points only, and those read the planes, the walls and the field
    c->have_explicit = true; c->c0_omega = NAN; c->have_walls = true;
    c->phase_mode = 0;
    c->have_matfree = false; dict_reset(c); c->wrap_links = false; c->native3 = false;
    adjoint_reset(c);
    v->have_system = true;
    return DEFF_OK;
}
DEFF_API_CATCH

// A[n * 7] = a0, aW, aE, aS, aN, aB, aF per cell, b[n]; n = nz * ny * nx (true width)
extern "C" int deff_volume_get_system(deff_volume *v, double *A, double *b)
try {
    if (!v || !A || !b) return fail(DEFF_EINVAL, "NULL argument");
    if (!v->have_system) return fail(DEFF_ESTATE, "no system assembled");
    deff_ctx *c = v->c;
    TRY(use_device(c));
    const size_t n = (size_t)c->nxt * c->rows;
    std::vector<double> plane(n);
    const double *planes[7] = {c->a0, c->aW, c->aE, c->aS, c->aN, v->aB, v->aF};
    for (int k = 0; k < 7; ++k) {
        TRY(rows_d2h(c, plane.data(), planes[k], (size_t)c->rows));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t p = 0; p < n; ++p) A[p * 7 + k] = plane[p];
    }
    TRY(rows_d2h(c, b, (const double *)c->b, (size_t)c->rows));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_volume_init_linear(deff_volume *v, double CL, double CR)
try {
    if (!v) return fail(DEFF_EINVAL, "volume is NULL");
    return deff_init_linear(v->c, CL, CR);
}
DEFF_API_CATCH

extern "C" int deff_volume_set_field(deff_volume *v, const double *x)
try {
    if (!v || !x) return fail(DEFF_EINVAL, "NULL argument");
    return deff_set_field(v->c, x);
}
DEFF_API_CATCH

extern "C" int deff_volume_get_field(deff_volume *v, double *x)
try {
    if (!v || !x) return fail(DEFF_EINVAL, "NULL argument");
    return deff_get_field(v->c, x);
}
DEFF_API_CATCH

extern "C" int deff_volume_device_field(deff_volume *v, void **d_x, size_t *pitch)
try {
    if (!v || !d_x) return fail(DEFF_EINVAL, "NULL argument");
    return deff_device_field(v->c, d_x, pitch);
}
DEFF_API_CATCH

extern "C" int deff_volume_flux(deff_volume *v, double *deff_raw, double *MFL, double *MFR)
try {
    if (!v || !deff_raw) return fail(DEFF_EINVAL, "NULL argument");
    return deff_flux(v->c, deff_raw, MFL, MFR);
}
DEFF_API_CATCH

extern "C" int deff_volume_solve_cg(deff_volume *v, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out,
                                    double *MFL, double *MFR)
try {
    if (!v || !out) return fail(DEFF_EINVAL, "NULL argument");
    if (!(rtol >= 0.0) || !std::isfinite(rtol)) return fail(DEFF_EINVAL, "deff_volume_solve_cg: rtol must be finite and >= 0");
    if (max_iter < 0) return fail(DEFF_EINVAL, "deff_volume_solve_cg: negative max_iter");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    if (!v->c->have_field) return fail(DEFF_ESTATE, "no field: call deff_volume_init_linear() or deff_volume_set_field()");
    if (!v->have_system) return fail(DEFF_ESTATE, "no system assembled: call deff_volume_assemble_from_D()");
    return volume_solve_cg(v->c, v->aB, v->aF, v->ny, rtol, max_iter, check_every, out, MFL, MFR);
}
DEFF_API_CATCH

// The Deff gradient of the volume's field.  Everything that can refuse the call comes before anything is touched; the pass
// (volume_sens_run, api_facepass.hip) writes the private context's pass_sens and the upload scratch, nothing else.
extern "C" int deff_volume_sensitivity_D(deff_volume *v, const double *D, double CL, double CR, double *g, double *euler, float *ms)
try {
    if (!v) return fail(DEFF_EINVAL, "volume is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    if (!v->c->have_field) return fail(DEFF_ESTATE, "no field");
    if (CR == CL) return fail(DEFF_EINVAL, "deff_volume_sensitivity_D: CR == CL (Deff is a flux per unit of CR - CL)");
    return volume_sens_run(v->c, D, v->ny, v->dy, v->dz, CL, CR, g, euler, ms);
}
DEFF_API_CATCH

extern "C" int deff_volume_device_sensitivity(deff_volume *v, void **d_map, size_t *row_pitch_bytes)
try {
    if (!v || !d_map) return fail(DEFF_EINVAL, "NULL argument");
    if (!v->c->pass_sens.have) return fail(DEFF_ESTATE, "no sensitivity map yet (deff_volume_sensitivity_D)");
    *d_map = v->c->pass_sens.map;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * v->c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_volume_set_tuning(deff_volume *v, const char *key, int value)
try {
    if (!v || !key) return fail(DEFF_EINVAL, "NULL argument");
    if (value < 0) return fail(DEFF_EINVAL, "tuning value must be >= 0");
    if (strcmp(key, "sens_kt")) return fail(DEFF_EINVAL, "deff_volume_set_tuning: unknown key '%s' (volumes take \"sens_kt\")", key);
    v->c->pass_sens.kt = value;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_volume_get_plan(deff_volume *v, const char *key, int *value)
try {
    if (!v || !key || !value) return fail(DEFF_EINVAL, "NULL argument");
    for (const char *k : {"cg_kr", "cg_items", "cg_restarts", "cg_impl", "sens_kt", "sens_items"})
        if (!strcmp(key, k)) return deff_get_plan(v->c, key, value);
    return fail(DEFF_EINVAL, "deff_volume_get_plan: unknown key '%s'", key);
}
DEFF_API_CATCH
