// api_flux.hip -- deff_flux_field / deff_flux_field_D / deff_device_flux_field: the flux through every face of the context's
// current field and the total flux through every vertical section, one pass on the device (kernels_flux.hpp).  Reads the
// field; changes nothing but its own maps, partial sums and the shared upload scratch.
#include "cell_pass.hpp"
#include "kernels_flux.hpp"
static_assert(FP_ROWS == CELL_PASS_ROWS && FP_COLS == CELL_PASS_COLS, "cell_pass_items plans the flux pass's tiles");

namespace deff {

__global__ __launch_bounds__(256) void k_flux(const double *__restrict__ x, const double *__restrict__ D, int nx, int nxt, int ny,
                                              int nimg, int ntx, int cpi, int kt, FluxGeom g, double CL, double CR,
                                              double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ left,
                                              double *__restrict__ colpart, double *__restrict__ wallpart)
{
    flux_pass(x, D, nx, nxt, ny, nimg, ntx, cpi, kt, g, CL, CR, fx, fy, left, colpart, wallpart);
}

__global__ __launch_bounds__(256) void k_flux_sections(const double *__restrict__ colpart, const double *__restrict__ wallpart,
                                                       int nx, int nxt, int nimg, int cpi, double *__restrict__ Q)
{
    flux_sections_body(colpart, wallpart, nx, nxt, nimg, cpi, Q);
}

}  // namespace deff

// Everything that can refuse the call, before anything is touched.
static int flux_common(deff_ctx *c, const char *who)
{
    TRY(slab_refused(c, who));
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(use_device(c));
    return DEFF_OK;
}

// the maps and sections of the stack's newest fields (x[cur] after consolidate) for the D plane `dD` on the device (pitch nx, pad column 0)
static int flux_launch(deff_ctx *c, const double *dD, double CL, double CR, double *fx, double *fy, double *left, double *sections,
                       float *ms)
{
    FluxPass &p = c->pass_flux;
    const CellItems it = cell_pass_items(c->nxt, c->ny, c->nimg, p.kt);
    if ((it.items + 3) / 4 > 0x7fffffffu) return fail(DEFF_EINVAL, "deff_flux_field: too many work items");
    const size_t nq = (size_t)c->nimg * ((size_t)c->nxt + 1), chunks = (size_t)c->nimg * it.cpi;
    TRY(flux_pass_room(c, p, chunks));
    TRY(cell_pass_start(c, p, ms));
    const FluxGeom g{c->dx, c->dy, c->dx / 2, c->dy / 2};
    hipLaunchKernelGGL(k_flux, dim3((unsigned)((it.items + 3) / 4)), dim3(256), 0, c->stream, c->x[c->cur], dD, c->nx, c->nxt,
                       c->ny, c->nimg, it.ntx, it.cpi, it.kt, g, CL, CR, p.fx, p.fy, p.left, p.colpart, p.wallpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_flux_sections, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, c->stream, p.colpart, p.wallpart, c->nx,
                       c->nxt, c->nimg, it.cpi, p.Q);
    HIP_TRY(hipGetLastError());
    TRY(cell_pass_launched(c, p, it, true, ms));
    if (fx) TRY(rows_d2h(c, fx, (const double *)p.fx, (size_t)c->rows));
    if (fy) TRY(rows_d2h(c, fy, (const double *)p.fy, (size_t)c->rows));
    if (left) HIP_TRY(hipMemcpyAsync(left, p.left, sizeof(double) * c->rows, hipMemcpyDeviceToHost, c->stream));
    if (sections) HIP_TRY(hipMemcpyAsync(sections, p.Q, sizeof(double) * nq, hipMemcpyDeviceToHost, c->stream));
    return cell_pass_wait(c, p, ms);
}

extern "C" int deff_flux_field_D(deff_ctx *c, const double *D, double CL, double CR, double *fx, double *fy, double *left,
                                 double *sections, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!D) return fail(DEFF_EINVAL, "D is NULL");
    TRY(flux_common(c, "deff_flux_field_D"));
    TRY(consolidate(c));                                           // every image's newest field in x[cur]
    const double *dD;
    TRY(cell_pass_upload_D(c, D, &dD));
    return flux_launch(c, dD, CL, CR, fx, fy, left, sections, ms);
}
DEFF_API_CATCH

extern "C" int deff_flux_field(deff_ctx *c, double *fx, double *fy, double *left, double *sections, float *ms)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    TRY(slab_refused(c, "deff_flux_field"));
    const double *dD;
    TRY(image_D_plane(c, "deff_flux_field", "its fluxes are", [c] {
        TRY(flux_common(c, "deff_flux_field"));
        return consolidate(c);
    }, &dD));
    return flux_launch(c, dD, c->CL, c->CR, fx, fy, left, sections, ms);
}
DEFF_API_CATCH

extern "C" int deff_device_flux_field(deff_ctx *c, void **d_fx, void **d_fy, size_t *row_pitch_bytes)
try {
    if (!c || !d_fx || !d_fy) return fail(DEFF_EINVAL, "NULL argument");
    if (!c->pass_flux.have) return fail(DEFF_ESTATE, "no flux field yet (deff_flux_field / deff_flux_field_D)");
    *d_fx = c->pass_flux.fx;
    *d_fy = c->pass_flux.fy;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}
DEFF_API_CATCH
