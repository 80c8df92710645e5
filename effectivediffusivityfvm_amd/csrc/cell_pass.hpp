// cell_pass.hpp -- the host path of a pass over the cells of the current field: the residual (api_residual.hip), the five face
// passes that end in one sum per image (api_facepass.hip) and the flux field (api_flux.hip).  Each entry point keeps its own
// refusals and its own kernel launch; what is here is what they do alike: the work-item planner, the buffers, the call's own
// event pair and plan keys, the final sum and the copies out, the D plane on the device -- a caller's, or the assembled
// image's -- and the device-map getter.
#pragma once
#include "ctx.hpp"

constexpr int CELL_PASS_ROWS = 8, CELL_PASS_COLS = 128;          // the tile of a wave in every kernel planned here

struct CellItems {
    int ntx, kt, cpi, nimg;         // column strips, tiles per work item, work items per strip and image, images of the launch
    size_t per_img, items;          // work items (= partial sums) per image and in the launch
};

// Work items: column strips of 128, cut into runs of kt tiles of 8 rows that one wave streams top to bottom (the rows above
// and below a run are then loaded once per run).  kt: about 4 096 items in the launch -- one round of waves on 256 CUs;
// measured with the residual's class kernel at 4096^2, reduction included: kt = 1 42.0 us, 2 34.4, 4 32.0, 8 31.7 -- and at most
// 16 384 items per image (the final kernel adds an image's partial sums with ONE workgroup); `tuned` > 0 (tuning "res_kt" /
// "sens_kt" / "vjp_kt" / "tan_kt" / "hvp_kt" / "fhvp_kt") overrides; clipped to the image.
static inline CellItems cell_pass_items(int nxt, int ny, int nimg, int tuned)
{
    const int ntx = (nxt + CELL_PASS_COLS - 1) / CELL_PASS_COLS, tiles_y = (ny + CELL_PASS_ROWS - 1) / CELL_PASS_ROWS;
    int kt = tuned;
    if (kt <= 0) {
        kt = (int)std::min<size_t>(64, std::max<size_t>(1, (size_t)ntx * tiles_y * nimg / 4096));
        kt = std::max(kt, (int)(((size_t)ntx * tiles_y + 16383) / 16384));
    }
    if (kt > tiles_y) kt = tiles_y;
    const int cpi = (tiles_y + kt - 1) / kt;
    const size_t per_img = (size_t)ntx * cpi;
    return CellItems{ntx, kt, cpi, nimg, per_img, per_img * nimg};
}

// Room for the map (if the pass has one) and for `partials` partial sums + one sum per image of the context.
static inline int cell_pass_room(deff_ctx *c, CellPass &p, bool with_map, size_t partials)
{
    if (with_map) TRY(dev_alloc(&p.map, c->n));
    const size_t want = partials + (size_t)c->nimg;
    if (p.part_cap < want) {
        if (p.part) { HIP_TRY(hipFree(p.part)); p.part = nullptr; p.part_cap = 0; }
        HIP_TRY(hipMalloc((void **)&p.part, want * sizeof(double)));
        p.part_cap = want;
    }
    return DEFF_OK;
}

// Opens the timed window of a call that asked for `ms`.
static inline int cell_pass_start(deff_ctx *c, PassPlan &p, const float *ms)
{
    if (!ms) return DEFF_OK;
    if (!p.ev0) HIP_TRY(hipEventCreate(&p.ev0));
    if (!p.ev1) HIP_TRY(hipEventCreate(&p.ev1));
    HIP_TRY(hipEventRecord(p.ev0, c->stream));
    return DEFF_OK;
}

// After a pass's last kernel: the end of the timed window, and what deff_get_plan reports of the launch.
static inline int cell_pass_launched(deff_ctx *c, PassPlan &p, const CellItems &it, bool have, const float *ms)
{
    if (ms) HIP_TRY(hipEventRecord(p.ev1, c->stream));
    p.have = have;
    p.plan_kt = it.kt; p.plan_items = (int)it.per_img;           // deff_get_plan "*_kt" / "*_items": what was launched
    return DEFF_OK;
}

// After the copies out were enqueued: waits for them, and reads the window's time.
static inline int cell_pass_wait(deff_ctx *c, PassPlan &p, float *ms)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, p.ev0, p.ev1));
    return DEFF_OK;
}

// After the pass's own kernel: the final sum of `it.per_img` partials for each of `it.nimg` images, the end of the timed
// window, and what the caller wants on the host -- the sums (it.nimg doubles) and the map (true width), each or neither.
static inline int cell_pass_finish(deff_ctx *c, CellPass &p, void (*final_kernel)(const double *, size_t, double *),
                                   const CellItems &it, double *sums, double *map, float *ms)
{
    double *out = p.part + it.items;
    hipLaunchKernelGGL(final_kernel, dim3(it.nimg), dim3(1024), 0, c->stream, p.part, it.per_img, out);
    HIP_TRY(hipGetLastError());
    TRY(cell_pass_launched(c, p, it, p.map != nullptr, ms));
    if (map) TRY(rows_d2h(c, map, (const double *)p.map, (size_t)c->rows));
    if (sums) HIP_TRY(hipMemcpyAsync(sums, out, sizeof(double) * it.nimg, hipMemcpyDeviceToHost, c->stream));
    return cell_pass_wait(c, p, ms);
}

// A caller's D plane (true width) in the shared upload scratch: pitch nx, pad column 0.  A pass that uploads `slots` planes
// (the tangent's and the Hessian-vector pass's D and dD) names the plane's slot; the scratch holds them one after the other.
static inline int cell_pass_upload_D(deff_ctx *c, const double *D, const double **dD, int slot = 0, int slots = 1)
{
    TRY(ensure_scratch(c, sizeof(double) * c->n * slots));
    double *d = (double *)c->scratch + (size_t)slot * c->n;
    TRY(plane_h2d(c, d, D));
    *dD = d;
    return DEFF_OK;
}

// The D plane of the system assembled from the image, in the shared upload scratch (pitch nx, pad column 0), for `who` =
// deff_sensitivity / deff_flux_field: is there such a plane? -- `what` completes the second refusal ("its Deff is", "its fluxes
// are") --, then `ready()`, the entry point's own refusals and its consolidate, which come between, then the fill from the pixels.
template <typename Ready>
static inline int image_D_plane(deff_ctx *c, const char *who, const char *what, Ready ready, const double **dD)
{
    if (!c->phase_mode || !c->have_image)
        return fail(DEFF_ESTATE, "%s needs a system assembled from the image (deff_assemble_2phase / _3phase); "
                                 "pass the diffusivities to %s_D() otherwise", who, who);
    if (c->native3 || (c->phase_mode == 3 && c->grid_given))
        return fail(DEFF_EINVAL, "%s: the system was assembled with a Grid (identity rows of the flood fill): "
                                 "%s not a function of the phase diffusivities alone", who, what);
    TRY(ready());
    TRY(ensure_scratch(c, sizeof(double) * c->n));
    double *d = (double *)c->scratch;
    if (c->phase_mode == 2)
        hipLaunchKernelGGL(k_fill_D_2phase, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                           c->nxt, c->ny, c->rows, c->phase_D[0], c->phase_D[1], d);
    else
        hipLaunchKernelGGL(k_fill_D_3phase, dim3(grid_for(c->n)), dim3(256), 0, c->stream, c->pix, c->W, c->ampX, c->ampY, c->nx,
                           c->nxt, c->ny, c->rows, c->phase_D[0], c->phase_D[1], c->phase_D[2], d);
    HIP_TRY(hipGetLastError());
    *dD = d;
    return DEFF_OK;
}

// deff_device_sensitivity and the four like it: the last map of pass `which`, or `none` as the message of DEFF_ESTATE.
static inline int cell_pass_device_map(deff_ctx *c, CellPass deff_ctx::*which, void **d_g, size_t *row_pitch_bytes, const char *none)
{
    if (!c || !d_g) return fail(DEFF_EINVAL, "NULL argument");
    if (!(c->*which).have) return fail(DEFF_ESTATE, "%s", none);
    *d_g = (c->*which).map;
    if (row_pitch_bytes) *row_pitch_bytes = sizeof(double) * c->nx;
    return DEFF_OK;
}

static inline void pass_plan_free(PassPlan &p)
{
    if (p.ev0) (void)hipEventDestroy(p.ev0);
    if (p.ev1) (void)hipEventDestroy(p.ev1);
}

static inline void cell_pass_free(CellPass &p)
{
    if (p.map) (void)hipFree(p.map);
    if (p.part) (void)hipFree(p.part);
    pass_plan_free(p);
}

// The flux field's buffers (api_flux.hip): the two maps, the left wall's rows, the section sums, and room for `chunks` work
// items' column sums (pitch nx) and left-wall sums.
static inline int flux_pass_room(deff_ctx *c, FluxPass &p, size_t chunks)
{
    TRY(dev_alloc(&p.fx, c->n));
    TRY(dev_alloc(&p.fy, c->n));
    TRY(dev_alloc(&p.left, (size_t)c->rows));
    TRY(dev_alloc(&p.Q, (size_t)c->nimg * ((size_t)c->nxt + 1)));
    if (p.part_cap < chunks) {
        if (p.colpart) { HIP_TRY(hipFree(p.colpart)); p.colpart = nullptr; }
        if (p.wallpart) { HIP_TRY(hipFree(p.wallpart)); p.wallpart = nullptr; }
        p.part_cap = 0;
        HIP_TRY(hipMalloc((void **)&p.colpart, chunks * (size_t)c->nx * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&p.wallpart, chunks * sizeof(double)));
        p.part_cap = chunks;
    }
    return DEFF_OK;
}

static inline void flux_pass_free(FluxPass &p)
{
    for (double *d : {p.fx, p.fy, p.left, p.colpart, p.wallpart, p.Q})
        if (d) (void)hipFree(d);
    pass_plan_free(p);
}
