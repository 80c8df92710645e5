// api_cg.hip -- deff_solve_cg: Jacobi-preconditioned conjugate gradients to a residual tolerance (kernels_cg.hpp; on the
// explicit coefficient planes for systems without a row dictionary, tuning key "cg_planes": kernels_cg_planes.hpp), and
// deff_solve_cg_stream: the same solve through the refilled slots of a stack (kernels_cg_stream.hpp, second half); at the end
// the steps of one row slab of deff_slab_*_solve_cg (kernels_cg_slab.hpp; the loop over the slabs is in api_slab.hip).  Not the
// reference's algorithm: it reaches the same discrete fixed point (same A, b, wall-flux Deff) as the weighted Jacobi loop of
// deff_solve, in far fewer iterations.  Nothing of the Jacobi path is touched: its tables (lut, c0 plane), plans and knobs
// stay as they are (the "fma" knob does not apply here: CG's arithmetic is written-order FP64 only).
// The launches of one iteration, in every form and under every fold key, are CgIteration::enqueue's, for both solves.
// deff_solve_adjoint (A lambda = w for the gradient of a loss on the field) and deff_solve_tangent (A dx = r for
// the field's derivative along a direction; both read by the passes of api_facepass.hip) run deff_solve_cg's host loop,
// cg_host_loop, on the coefficient planes with its own solution and right-hand side buffers.  Under the tuning key
// "cg_onchip_planes" every solve on the planes iterates small images on one compute unit each (kernels_cg_image_planes.hpp).
// A volume (api_volume.hip) is the plane form on one tall image plus the z links: its kernels (kernels_cg_volume.hpp) are
// launched here, from volume_assemble_planes and volume_solve_cg, and the loop takes them through CgIteration::z.
#include "ctx.hpp"
#include "kernels_cg.hpp"
#include "kernels_cg_planes.hpp"
#include "kernels_cg_volume.hpp"
#include "kernels_cg_fold.hpp"
#include "kernels_cg_image.hpp"
#include "kernels_cg_image_planes.hpp"
#include "kernels_cg_stream.hpp"
#include "kernels_cg_slab.hpp"
#include "cg_slab.hpp"
#include <vector>

// (CG_MAX_RESTARTS, cg_slab.hpp: true-residual rounds that may restart the recurrence of a finished image; each round costs
// one pass and a synchronisation)

// CG table from the host dictionary: planes A0, 1/A0, aW, aE, aS, aN, b; decoupled rows (four zero links, b == 0) stay all
// zeros.  An active row must have a finite positive A0 with a normal 1/A0 and finite links and b.
static int cg_table(const std::vector<double> &rows, int nrows, std::vector<double> &t)
{
    t.assign(CG_DOUBLES, 0.0);
    constexpr int S = LUT_PLANE_STRIDE;
    for (int k = 1; k < nrows; ++k) {
        const double *row = &rows[(size_t)k * 6];
        const double a0 = row[0], aW = row[1], aE = row[2], aS = row[3], aN = row[4], b = row[5];
        if (aW == 0.0 && aE == 0.0 && aS == 0.0 && aN == 0.0 && b == 0.0) continue;   // decoupled: x = 0
        const double inv = 1.0 / a0;
        if (!(a0 > 0.0) || !std::isnormal(inv) || !std::isfinite(a0) || !std::isfinite(aW) || !std::isfinite(aE) ||
            !std::isfinite(aS) || !std::isfinite(aN) || !std::isfinite(b))
            return fail(DEFF_EINVAL, "deff_solve_cg: matrix row %d (A0 = %g, links %g %g %g %g, b = %g) is not admissible: "
                                     "an active row needs a finite A0 > 0 and finite links",
                        k, a0, aW, aE, aS, aN, b);
        t[(size_t)CG_A0 * S + k] = a0;
        t[(size_t)CG_INV * S + k] = inv;
        t[(size_t)CG_W * S + k] = aW;
        t[(size_t)CG_E * S + k] = aE;
        t[(size_t)CG_S * S + k] = aS;
        t[(size_t)CG_N * S + k] = aN;
        t[(size_t)CG_B * S + k] = b;
    }
    return DEFF_OK;
}

static int cg_table(const deff_ctx *c, std::vector<double> &t) { return cg_table(c->lut_rows, c->lut_nrows, t); }

// rows per work item of an image of `ntx` strips and ny rows: ~8 192 items per image, 2..16 rows each
static int cg_rows_per_item(int ntx, int ny) { return (int)std::max(2L, std::min(16L, (long)ntx * ny / 8192)); }

// Work items of one image: strips of 128 columns x kr rows, kr chosen from (nx, ny) alone so that an image of a stack is cut
// (and its sums ordered) exactly like a one-image context's.
static CgGeom cg_geometry(const deff_ctx *c)
{
    CgGeom g;
    g.nx = c->nx;
    g.ny = c->ny;
    g.nimg = c->nimg;
    g.ntx = (c->nx + CG_COLS - 1) / CG_COLS;
    g.kr = cg_rows_per_item(g.ntx, c->ny);
    g.cpi = (c->ny + g.kr - 1) / g.kr;
    g.per_img = (unsigned)((size_t)g.ntx * g.cpi);
    return g;
}

// one workgroup per image (kernels_cg_image.hpp, kernels_cg_image_planes.hpp): the form's own tuning key is set and an image's
// cells fit a compute unit
static bool cg_onchip_form(const deff_ctx *c, bool planes)
{
    return (planes ? c->cg_onchip_planes : c->cg_onchip) && (size_t)c->nx * c->ny <= (size_t)CGI_CELLS;
}

static int cg_buffers(deff_ctx *c, size_t items)
{
    if (!c->cg_r) {
        TRY(dev_alloc(&c->cg_r, c->n));
        TRY(dev_alloc(&c->cg_p[0], c->n));
        TRY(dev_alloc(&c->cg_p[1], c->n));
        HIP_TRY(hipMemsetAsync(c->cg_p[0], 0, sizeof(double) * c->n, c->stream));
        HIP_TRY(hipMemsetAsync(c->cg_p[1], 0, sizeof(double) * c->n, c->stream));
        TRY(dev_alloc(&c->cg_tab, (size_t)CG_DOUBLES));
        TRY(dev_alloc(&c->cg_flags, 2));
        if (hipMalloc(&c->cg_scal, sizeof(CgScal) * c->nimg) != hipSuccess) return fail(DEFF_ENOMEM, "deff_solve_cg: scalars");
        HIP_TRY(hipEventCreate(&c->cg_ev0));
        HIP_TRY(hipEventCreate(&c->cg_ev1));
    }
    if (c->cg_part_cap < 3 * items) {
        if (c->cg_part) { HIP_TRY(hipFree(c->cg_part)); c->cg_part = nullptr; c->cg_part_cap = 0; }
        HIP_TRY(hipMalloc((void **)&c->cg_part, sizeof(double) * 3 * items));
        c->cg_part_cap = 3 * items;
    }
    // arrival counters of the folded launches ("cg_fold"): one set for the direction launch, one for the update launch
    const size_t ticks = 2 * cgf_ticks((unsigned)(items / std::max(1, c->nimg)), (size_t)c->nimg);
    if (c->cg_tick_cap < ticks) {
        if (c->cg_tick) { HIP_TRY(hipFree(c->cg_tick)); c->cg_tick = nullptr; c->cg_tick_cap = 0; }
        HIP_TRY(hipMalloc((void **)&c->cg_tick, sizeof(unsigned) * ticks));
        c->cg_tick_cap = ticks;
    }
    return DEFF_OK;
}

// the plane form's own work vectors (kernels_cg_planes.hpp): 1 / a0 per cell and q = A p
static int cgp_buffers(deff_ctx *c)
{
    TRY(dev_alloc(&c->cg_inv, c->n));
    TRY(dev_alloc(&c->cg_q, c->n));
    return DEFF_OK;
}

// One CG iteration on the context's stream: four launches, or two with the reductions folded in (fold 1, 2: tuning "cg_fold",
// kernels_cg_fold.hpp), on the row table or on the coefficient planes.  What does not change from one iteration to the next
// is set once per call; p_in / p_out swap.  Returns the number of launches.
struct CgIteration {
    deff_ctx *c;
    bool planes;
    int fold;
    dim3 grid, fin;
    CgGeom g;
    double *x, *part, *part_rz, *part_rr;
    unsigned *tick_a, *tick_b;
    double tol2;
    long long max_iter;
    const double *rhs = nullptr;    // plane form: the right-hand side plane (the iteration's kernels read the matrix planes only)
    CgvLinks z = CgvLinks();        // plane form of a volume (kernels_cg_volume.hpp): the z links and the slice's rows; z.ny = 0 otherwise

    int enqueue(const double *p_in, double *p_out) const
    {
        const CgpPlanes P{c->a0, c->aW, c->aE, c->aS, c->aN, rhs};
        CgScal *sc = (CgScal *)c->cg_scal;
        if (fold) {
            if (planes) {
                hipLaunchKernelGGL(k_cgpf_dir, grid, dim3(256), 0, c->stream, P, c->cg_inv, c->cg_r, p_in, p_out, c->cg_q, sc, g,
                                   part, tick_a);
                hipLaunchKernelGGL(k_cgpf_update, grid, dim3(256), 0, c->stream, c->cg_inv, p_out, c->cg_q, x, c->cg_r, sc, g,
                                   part_rz, part_rr, tol2, max_iter, tick_b);
            } else {
                hipLaunchKernelGGL(fold == 2 ? k_cgf_dir2 : k_cgf_dir, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows,
                                   c->code, c->cg_r, p_in, p_out, sc, g, part, tick_a);
                hipLaunchKernelGGL(k_cgf_update, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, p_out, x,
                                   c->cg_r, sc, g, part_rz, part_rr, tol2, max_iter, tick_b);
            }
            return 2;
        }
        if (z.ny)
            hipLaunchKernelGGL(k_cgv_dir, grid, dim3(256), 0, c->stream, P, z, c->cg_inv, c->cg_r, p_in, p_out, c->cg_q, sc, g, part);
        else if (planes)
            hipLaunchKernelGGL(k_cgp_dir, grid, dim3(256), 0, c->stream, P, c->cg_inv, c->cg_r, p_in, p_out, c->cg_q, sc, g, part);
        else
            hipLaunchKernelGGL(k_cg_dir, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, c->cg_r, p_in, p_out, sc,
                               g, part);
        hipLaunchKernelGGL(k_cg_alpha, fin, dim3(CG_FIN), 0, c->stream, part, g.per_img, sc);
        if (planes)
            hipLaunchKernelGGL(k_cgp_update, grid, dim3(256), 0, c->stream, c->cg_inv, p_out, c->cg_q, x, c->cg_r, sc, g, part_rz,
                               part_rr);
        else
            hipLaunchKernelGGL(k_cg_update, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, p_out, x, c->cg_r, sc,
                               g, part_rz, part_rr);
        hipLaunchKernelGGL(k_cg_beta, fin, dim3(CG_FIN), 0, c->stream, part_rz, part_rr, g.per_img, sc, tol2, max_iter);
        return 4;
    }
};

// The host loop of a CG solve, for deff_solve_cg (x = the field, rhs = the b plane) and deff_solve_adjoint (x = lambda,
// rhs = w'): the start's true residual, check_every iterations between two looks at the images' flags, the true-residual
// rounds at the end.  The caller has prepared the table or cg_inv, zeroed cg_flags and cg_tick and set the "cg_*" plan keys;
// `planes` reads the matrix from the coefficient planes and the right-hand side from `rhs` (the table form has b in its
// table and ignores it).  hs[img] = the images' final scalars, *ms = the loop's time on cg_ev0 / cg_ev1.
// A volume (volume_solve_cg below: planes, neither on chip nor folded) passes its z links: the direction and the residual
// launch are then the volume's kernels, everything else is as for an image of ny * nz rows.
static int cg_host_loop(deff_ctx *c, double *x, const double *rhs, bool planes, bool onchip, int fold, const CgGeom &g,
                        double rtol, int64_t max_iter, int64_t check_every, std::vector<CgScal> &hs, float *ms,
                        const CgvLinks &z = CgvLinks())
{
    const size_t items = (size_t)g.per_img * c->nimg;
    const CgpPlanes P{c->a0, c->aW, c->aE, c->aS, c->aN, rhs};
    unsigned flag1 = 0;
    const double tol2 = rtol * rtol;
    const dim3 grid((unsigned)((items + 3) / 4)), fin((unsigned)c->nimg);
    double *part = c->cg_part, *part_rz = c->cg_part + items, *part_rr = c->cg_part + 2 * items;
    CgScal *sc = (CgScal *)c->cg_scal;
    const CgIteration iteration{c, planes, fold, grid, fin, g, x, part, part_rz, part_rr, c->cg_tick,
                                c->cg_tick + cgf_ticks(g.per_img, (size_t)c->nimg), tol2, (long long)max_iter, rhs, z};
    hs.resize(c->nimg);
    auto true_residual = [&](int mode, int allow) -> int {
        if (z.ny) hipLaunchKernelGGL(k_cgv_resid, grid, dim3(256), 0, c->stream, P, z, c->cg_inv, x, c->cg_r, g, part);
        else if (planes) hipLaunchKernelGGL(k_cgp_resid, grid, dim3(256), 0, c->stream, P, c->cg_inv, x, c->cg_r, g, part);
        else hipLaunchKernelGGL(k_cg_resid, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, x, c->cg_r, g, part);
        hipLaunchKernelGGL(k_cg_check, fin, dim3(CG_FIN), 0, c->stream, part, g.per_img, sc, tol2, (long long)max_iter, mode,
                           allow, c->cg_flags + 1);
        HIP_TRY(hipGetLastError());
        return DEFF_OK;
    };
    HIP_TRY(hipEventRecord(c->cg_ev0, c->stream));
    TRY(true_residual(0, 0));
    int64_t k = 0;                                                   // iterations enqueued (parity of the p buffers)
    int rounds = 0;
    for (;;) {
        HIP_TRY(hipMemcpyAsync(hs.data(), sc, sizeof(CgScal) * c->nimg, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        bool all_done = true;
        for (const CgScal &s : hs) all_done &= s.done != 0;
        if (all_done) {
            // the recurrence's residual drifts from b - A x: recompute it; an image whose true residual misses rtol goes on
            HIP_TRY(hipMemsetAsync(c->cg_flags + 1, 0, sizeof(unsigned), c->stream));
            TRY(true_residual(1, rounds < CG_MAX_RESTARTS));
            HIP_TRY(hipMemcpyAsync(&flag1, c->cg_flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(hs.data(), sc, sizeof(CgScal) * c->nimg, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (flag1 == 0) break;
            ++rounds;
            c->cg_plan_restarts = rounds;
        }
        if (onchip) {
            // up to check_every iterations of every running image, p in cg_p[0] throughout (the streaming loop below starts
            // every call at cg_p[0] with the restart flag set, so the forms never read each other's p); on the planes
            // (tuning "cg_onchip_planes") the same launch of k_cgp_image, which reads the matrix planes and cg_inv only
            const dim3 wgs((unsigned)std::min(c->nimg, c->cg_cus));
            if (planes)
                hipLaunchKernelGGL(k_cgp_image, wgs, dim3(CGI_THREADS), 0, c->stream, P, c->cg_inv, x, c->cg_r, c->cg_p[0], sc, c->nx,
                                   c->ny, c->nimg, (long long)check_every, tol2, (long long)max_iter);
            else
                hipLaunchKernelGGL(k_cg_image, wgs, dim3(CGI_THREADS), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, x, c->cg_r,
                                   c->cg_p[0], sc, c->nx, c->ny, c->nimg, (long long)check_every, tol2, (long long)max_iter);
            HIP_TRY(hipGetLastError());
            continue;
        }
        for (int64_t i = 0; i < check_every; ++i, ++k) iteration.enqueue(c->cg_p[k & 1], c->cg_p[(k + 1) & 1]);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->cg_ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->cg_ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->cg_ev0, c->cg_ev1));
    return DEFF_OK;
}

extern "C" int deff_solve_cg(deff_ctx *c, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out,
                             double *MFL, double *MFR)
try {
    if (!c || !out) return fail(DEFF_EINVAL, "NULL argument");
    if (!(rtol >= 0.0) || !std::isfinite(rtol)) return fail(DEFF_EINVAL, "deff_solve_cg: rtol must be finite and >= 0");
    if (max_iter < 0) return fail(DEFF_EINVAL, "deff_solve_cg: negative max_iter");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    if (c->slab)
        return fail(DEFF_EINVAL, "deff_solve_cg: not for row-slab contexts (CG over row slabs sums over all slabs: call "
                                 "deff_slab_group_solve_cg or deff_slab_rank_solve_cg)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field: call deff_init_linear() or deff_set_field()");
    if (!c->have_walls) return fail(DEFF_ESTATE, "wall diffusivities unknown (needed for Deff)");
    if (c->wrap_links)
        return fail(DEFF_EINVAL, "deff_solve_cg: the system links a wall column to the neighbouring row (explicit-only system)");
    TRY(use_device(c));
    TRY(consolidate(c));                                             // every image's newest field in x[cur]
    // the form: the row table, or (tuning "cg_planes") the explicit coefficient planes -- 2 = always, 1 = when the system has no
    // dictionary after ensure_dictionary has had its try
    bool planes = c->cg_planes == 2;
    if (!planes) {
        if (!c->have_matfree && c->have_explicit) TRY(ensure_dictionary(c));
        if (!c->have_matfree) {
            if (c->cg_planes != 1 || !c->have_explicit)
                return fail(DEFF_EINVAL, "deff_solve_cg: the system has no row dictionary (too many distinct rows, or dictionaries "
                                         "disabled): CG runs on the matrix-free form only (the tuning key \"cg_planes\" lets it "
                                         "run on the coefficient planes)");
            planes = true;
        }
    }
    std::vector<double> tab;
    if (planes) TRY(explicit_from_image(c));                         // a native system's planes; nothing to do for any other
    else TRY(cg_table(c, tab));
    const CgGeom g = cg_geometry(c);
    const size_t items = (size_t)g.per_img * c->nimg;
    // on chip (tuning "cg_onchip"): an image whose arrays fit one compute unit's LDS and registers iterates there, one
    // launch per check_every iterations instead of four per iteration; larger images keep the streaming kernels
    // (on the planes: tuning "cg_onchip_planes", k_cgp_image)
    const bool onchip = cg_onchip_form(c, planes);
    if (onchip && !c->cg_cus) HIP_TRY(hipDeviceGetAttribute(&c->cg_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    TRY(cg_buffers(c, items));
    if (planes) TRY(cgp_buffers(c));
    c->cg_plan_kr = g.kr;
    c->cg_plan_ntx = g.ntx;
    c->cg_plan_items = (int)g.per_img;
    c->cg_plan_restarts = 0;
    c->cg_plan_impl = planes ? (onchip ? 4 : 3) : onchip ? 2 : 1;
    // two launches per iteration (tuning "cg_fold", kernels_cg_fold.hpp); the plane form's direction kernel loads ahead already
    const int fold = onchip ? 0 : (planes && c->cg_fold == 2) ? 1 : c->cg_fold;
    c->cg_plan_fold = fold;
    const CgpPlanes P{c->a0, c->aW, c->aE, c->aS, c->aN, c->b};

    // admissibility: active rows positive and finite (table form: cg_table above), active links symmetric bit for bit, no link
    // out of the image; nothing is changed on a refusal
    unsigned flags[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
    // the counters start every call at 0: the last arriver's reset alone would not do after a call that ended early
    HIP_TRY(hipMemsetAsync(c->cg_tick, 0, sizeof(unsigned) * 2 * cgf_ticks(g.per_img, (size_t)c->nimg), c->stream));
    if (planes)
        hipLaunchKernelGGL(k_cgp_prepare, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, P, c->nx, c->rows, c->ny, c->cg_inv,
                           c->cg_flags);
    else {
        HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), sizeof(double) * CG_DOUBLES, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_cg_admissible, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code,
                           c->nx, c->rows, c->ny, c->cg_flags);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags, c->cg_flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[0] & CGP_FLAG_ROW)
        return fail(DEFF_EINVAL, "deff_solve_cg: a matrix row is not admissible: an active row needs a finite A0 > 0 and finite "
                                 "links");
    if (flags[0])
        return fail(DEFF_EINVAL, "deff_solve_cg: the system is not symmetric (a link between two active cells differs from "
                                 "its partner, or an active row links out of its image)");

    std::vector<CgScal> hs;
    float ms = 0;
    TRY(cg_host_loop(c, c->x[c->cur], c->b, planes, onchip, fold, g, rtol, max_iter, check_every, hs, &ms));

    // Deff and wall fluxes of the final field: the same evaluation as deff_flux
    std::vector<double> deff(c->nimg);
    TRY(deff_flux(c, deff.data(), MFL, MFR));
    for (int i = 0; i < c->nimg; ++i) {
        out[i].iters = hs[i].iters;
        out[i].rel_residual = hs[i].rel;
        out[i].deff_raw = deff[i];
        out[i].loop_ms = ms;
        out[i].converged = hs[i].rel <= rtol;
    }
    return DEFF_OK;
}
DEFF_API_CATCH

// ---- volumes (api_volume.hip, kernels_cg_volume.hpp) ---------------------------------------------------------------------
//
// A deff_volume's private context is one image of nx x (ny * nz); these two run the volume's kernels on it.  They live here,
// beside the loop and the plane kernels they share: a kernel header is compiled into one translation unit.

// The eight planes of the 7-point system from the D volume in `dD` (device, pitch c->nx) and the wall diffusivities.
int volume_assemble_planes(deff_ctx *c, const double *dD, int ny, int nz, double dy, double dz, double CL, double CR, double *aB,
                           double *aF)
{
    hipLaunchKernelGGL(k_assemble_volume_from_D, dim3(grid_for(c->n)), dim3(256), 0, c->stream, dD, c->nx, c->nxt, ny, nz, c->dx, dy,
                       dz, CL, CR, soa_of(c), aB, aF);
    hipLaunchKernelGGL(k_wall_D_from_D, dim3((c->rows + 255) / 256), dim3(256), 0, c->stream, dD, c->nx, c->nxt, c->rows, c->Dl,
                       c->Dr);
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

// deff_solve_cg's plane form on a volume: the same checks on the system before the field is touched (k_cgv_prepare), the same
// loop, Deff and wall fluxes of the final field.  The caller has checked the arguments and the context's state.
int volume_solve_cg(deff_ctx *c, const double *aB, const double *aF, int ny, double rtol, int64_t max_iter, int64_t check_every,
                    deff_cg_result *out, double *MFL, double *MFR)
{
    TRY(use_device(c));
    const CgGeom g = cg_geometry(c);
    TRY(cg_buffers(c, g.per_img));
    TRY(cgp_buffers(c));
    c->cg_plan_kr = g.kr;
    c->cg_plan_ntx = g.ntx;
    c->cg_plan_items = (int)g.per_img;
    c->cg_plan_restarts = 0;
    c->cg_plan_impl = 5;
    c->cg_plan_fold = 0;
    const CgpPlanes P{c->a0, c->aW, c->aE, c->aS, c->aN, c->b};
    CgvLinks z;
    z.aB = aB;
    z.aF = aF;
    z.ny = ny;

    unsigned flags[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
    hipLaunchKernelGGL(k_cgv_prepare, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, P, z, c->nx, c->rows, c->cg_inv,
                       c->cg_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags, c->cg_flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[0] & CGP_FLAG_ROW)
        return fail(DEFF_EINVAL, "deff_volume_solve_cg: a matrix row is not admissible: an active row needs a finite A0 > 0 and "
                                 "finite links");
    if (flags[0])
        return fail(DEFF_EINVAL, "deff_volume_solve_cg: the system is not symmetric (a link between two active cells differs from "
                                 "its partner, or an active row links out of the volume)");

    std::vector<CgScal> hs;
    float ms = 0;
    TRY(cg_host_loop(c, c->x[c->cur], c->b, true, false, 0, g, rtol, max_iter, check_every, hs, &ms, z));
    double deff = 0;
    TRY(deff_flux(c, &deff, MFL, MFR));
    out->iters = hs[0].iters;
    out->rel_residual = hs[0].rel;
    out->deff_raw = deff;
    out->loop_ms = ms;
    out->converged = hs[0].rel <= rtol;
    return DEFF_OK;
}

// ---- deff_solve_adjoint, deff_solve_tangent, deff_solve_adjoint_tangent -----------------------------------------------------
//
// A lambda = w on the current matrix (symmetric: the adjoint system of A x = b is the same A), for the gradient of a loss on
// the field, A dx = r on it for the field's derivative along a direction of D, and A dlambda = q for lambda's (the passes that
// read and feed them: api_facepass.hip).  The plane form of deff_solve_cg with two pointers changed: the solution is the side
// vector's x (SideVec, ctx.hpp) instead of the field, the right-hand side its rhs -- w (r, q), zeroed where the FORWARD
// system's row is decoupled: cg_inv == 0 -- instead of the b plane.  cg_inv and the admissibility verdict are k_cgp_prepare's
// on the forward planes, b included.  Nothing the forward solve or the Jacobi path reads is written.  The entry points differ
// in the vector and in where the right-hand side comes from (the host; the last map of a pass, on the device).

// the arguments and the context's form: before any device work
static int side_solve_args(deff_ctx *c, const char *who, double rtol, int64_t max_iter, int64_t check_every)
{
    if (!(rtol >= 0.0) || !std::isfinite(rtol)) return fail(DEFF_EINVAL, "%s: rtol must be finite and >= 0", who);
    if (max_iter < 0) return fail(DEFF_EINVAL, "%s: negative max_iter", who);
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    TRY(slab_refused(c, who));
    if (c->wrap_links)
        return fail(DEFF_EINVAL, "%s: the system links a wall column to the neighbouring row (explicit-only system)", who);
    if (!c->have_explicit && !c->have_matfree) return fail(DEFF_ESTATE, "no system assembled");
    return DEFF_OK;
}

// the planes, the CG buffers, cg_inv and the verdict on the matrix; a refusal has changed nothing a caller can see
static int side_solve_prepare(deff_ctx *c, const char *who, CgGeom *geom)
{
    TRY(use_device(c));
    TRY(resident_check(c));                                          // the scratch and the stream are about to be used
    TRY(explicit_from_image(c));                                     // a native system's planes; nothing to do for any other
    const CgGeom g = cg_geometry(c);
    const size_t items = (size_t)g.per_img * c->nimg;
    TRY(cg_buffers(c, items));
    TRY(cgp_buffers(c));
    const CgpPlanes P{c->a0, c->aW, c->aE, c->aS, c->aN, c->b};

    unsigned flags[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
    HIP_TRY(hipMemsetAsync(c->cg_tick, 0, sizeof(unsigned) * 2 * cgf_ticks(g.per_img, (size_t)c->nimg), c->stream));
    hipLaunchKernelGGL(k_cgp_prepare, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, P, c->nx, c->rows, c->ny, c->cg_inv,
                       c->cg_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags, c->cg_flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[0] & CGP_FLAG_ROW)
        return fail(DEFF_EINVAL, "%s: a matrix row is not admissible: an active row needs a finite A0 > 0 and finite links", who);
    if (flags[0])
        return fail(DEFF_EINVAL, "%s: the system is not symmetric (a link between two active cells differs from its partner, or "
                                 "an active row links out of its image)", who);
    *geom = g;
    return DEFF_OK;
}

// the "cg_*" plan keys, and what every such solve does once its right-hand side is in `rhs`: the mask, the guess 0, the loop
static int side_solve_run(deff_ctx *c, double *x, double *rhs, const CgGeom &g, double rtol, int64_t max_iter,
                          int64_t check_every, deff_cg_result *out)
{
    c->cg_plan_kr = g.kr;
    c->cg_plan_ntx = g.ntx;
    c->cg_plan_items = (int)g.per_img;
    c->cg_plan_restarts = 0;
    const bool onchip = cg_onchip_form(c, true);
    if (onchip && !c->cg_cus) HIP_TRY(hipDeviceGetAttribute(&c->cg_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->cg_plan_impl = onchip ? 4 : 3;
    const int fold = onchip ? 0 : c->cg_fold == 2 ? 1 : c->cg_fold;
    c->cg_plan_fold = fold;
    hipLaunchKernelGGL(k_cgp_mask_rhs, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, c->cg_inv, c->n, rhs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(x, 0, sizeof(double) * c->n, c->stream));              // the guess, always

    std::vector<CgScal> hs;
    float ms = 0;
    TRY(cg_host_loop(c, x, rhs, true, onchip, fold, g, rtol, max_iter, check_every, hs, &ms));
    for (int i = 0; i < c->nimg; ++i) {
        out[i].iters = hs[i].iters;
        out[i].rel_residual = hs[i].rel;
        out[i].deff_raw = 0.0;                                       // neither lambda nor dx has a flux
        out[i].loop_ms = ms;
        out[i].converged = hs[i].rel <= rtol;
    }
    return DEFF_OK;
}

// One side solve into `v`: the right-hand side is the caller's plane `host_rhs` (true width), or -- host_rhs NULL -- the last map
// of pass `rhs_map`, copied on the device (the map itself stays as it was: the mask is applied to the copy), which has to have
// been computed for what `v` depends on (`no_rhs` otherwise).  With the same numbers in the right-hand side the three entry
// points below run the same arithmetic, bit for bit.
static int side_solve(deff_ctx *c, const char *who, SideVec &v, const double *host_rhs, const CellPass *rhs_map, const char *no_rhs,
                      double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out)
{
    TRY(side_solve_args(c, who, rtol, max_iter, check_every));
    if (!host_rhs && (!rhs_map->have || !v.rhs_ok)) return fail(DEFF_ESTATE, "%s: %s", who, no_rhs);
    CgGeom g;
    TRY(side_solve_prepare(c, who, &g));
    TRY(dev_alloc(&v.x, c->n));
    TRY(dev_alloc(&v.rhs, c->n));
    v.valid = false;                                                 // from here on the solution is the new call's
    if (&v == &c->adj) adjoint_tangent_reset(c);                     // ... and dlambda belonged to the old lambda
    if (host_rhs)
        TRY(plane_h2d(c, v.rhs, host_rhs));
    else
        HIP_TRY(hipMemcpyAsync(v.rhs, rhs_map->map, sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
    TRY(side_solve_run(c, v.x, v.rhs, g, rtol, max_iter, check_every, out));
    v.valid = true;
    return DEFF_OK;
}

extern "C" int deff_solve_adjoint(deff_ctx *c, const double *w, double rtol, int64_t max_iter, int64_t check_every,
                                  deff_cg_result *out)
try {
    if (!c || !w || !out) return fail(DEFF_EINVAL, "NULL argument");
    return side_solve(c, "deff_solve_adjoint", c->adj, w, nullptr, nullptr, rtol, max_iter, check_every, out);
}
DEFF_API_CATCH

// A dx = r', r the last deff_tangent_rhs_D's map.
extern "C" int deff_solve_tangent(deff_ctx *c, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out)
try {
    if (!c || !out) return fail(DEFF_EINVAL, "NULL argument");
    return side_solve(c, "deff_solve_tangent", c->tan, nullptr, &c->pass_tan,
                      "no right-hand side for the current system (deff_tangent_rhs_D)", rtol, max_iter, check_every, out);
}
DEFF_API_CATCH

// A dlambda = q' for the second-order field adjoint, q the last deff_adjoint_tangent_rhs_D's map.
extern "C" int deff_solve_adjoint_tangent(deff_ctx *c, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out)
try {
    if (!c || !out) return fail(DEFF_EINVAL, "NULL argument");
    return side_solve(c, "deff_solve_adjoint_tangent", c->atan, nullptr, &c->pass_atan,
                      "no right-hand side for the current system and adjoint field (deff_adjoint_tangent_rhs_D)", rtol, max_iter,
                      check_every, out);
}
DEFF_API_CATCH

// ---- deff_solve_cg_stream -----------------------------------------------------------------------------------------------
//
// The slot life cycle of deff_solve_stream around the CG iteration: every slot of a stack context iterates its own image,
// stops by its own rule on the device, has its true residual checked (and is sent back, up to CG_MAX_RESTARTS times, when it
// misses rtol) and is refilled with the next image -- while the other slots go on.  Per image the arithmetic is that of a
// one-image deff_solve_cg from the linear guess (kernels_cg_stream.hpp, "Determinism").
//
// The GPU does not wait for the host: the iteration work of interval i + 1 (one k_cg_image launch, or check_every x 4
// streaming launches) is enqueued BEFORE the host looks at the slot states interval i left behind; those arrive through an
// asynchronous copy into pinned memory and an event.  A slot found stopped is frozen (every iteration kernel skips it), so
// its true-residual round, flux, `done` callback, upload and entry kernels queue up behind interval i + 1 and the slot
// rejoins at interval i + 2; until then the snapshots still show its old state and are not read for it (`valid_from`).
// Launches and waits per interval do not depend on how many slots retire or enter: the slot-list kernels take them all.

namespace {

struct CgsBuffers {                                    // views into c->cgs_dev / c->cgs_pin
    int *d_fin, *d_rounds, *d_new;                     // device: the round's list, restart rounds per slot, the entering list
    uint8_t *d_pix;                                    // ... followed by the entering images' pixels (one H2D copy for both)
    int *h_fin, *h_new;
    uint8_t *h_pix;
    CgScal *h_snap[2];
    unsigned *h_flags[2];
    CgScal *h_round;
    double *h_q;
};

size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

int cgs_buffers(deff_ctx *c, size_t npix, CgsBuffers *b)
{
    const size_t B = (size_t)c->nimg;
    const size_t stage = round16(sizeof(int) * B + npix * B);
    const size_t dev = round16(sizeof(int) * B) * 2 + stage;
    const size_t snap = sizeof(CgScal) * B + 16;
    const size_t pin = round16(sizeof(int) * B) + stage + 2 * snap + sizeof(CgScal) * B + sizeof(double) * 2 * B;
    if (c->cgs_dev_bytes < dev) {
        if (c->cgs_dev) { HIP_TRY(hipFree(c->cgs_dev)); c->cgs_dev = nullptr; c->cgs_dev_bytes = 0; }
        HIP_TRY(hipMalloc(&c->cgs_dev, dev));
        c->cgs_dev_bytes = dev;
    }
    if (c->cgs_pin_bytes < pin) {
        if (c->cgs_pin) { HIP_TRY(hipHostFree(c->cgs_pin)); c->cgs_pin = nullptr; c->cgs_pin_bytes = 0; }
        HIP_TRY(hipHostMalloc(&c->cgs_pin, pin));
        c->cgs_pin_bytes = pin;
    }
    for (hipEvent_t &e : c->cgs_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    char *d = (char *)c->cgs_dev, *h = (char *)c->cgs_pin;
    b->d_fin = (int *)d;
    b->d_rounds = (int *)(d + round16(sizeof(int) * B));
    b->d_new = (int *)(d + 2 * round16(sizeof(int) * B));
    b->d_pix = (uint8_t *)(b->d_new + B);
    b->h_fin = (int *)h;
    b->h_new = (int *)(h + round16(sizeof(int) * B));
    b->h_pix = (uint8_t *)(b->h_new + B);
    h += round16(sizeof(int) * B) + stage;
    for (int k = 0; k < 2; ++k) {
        b->h_snap[k] = (CgScal *)h;
        b->h_flags[k] = (unsigned *)(h + sizeof(CgScal) * B);
        h += snap;
    }
    b->h_round = (CgScal *)h;
    b->h_q = (double *)(h + sizeof(CgScal) * B);
    return DEFF_OK;
}

}  // namespace

extern "C" int deff_solve_cg_stream(deff_ctx *c, int W, int H, int ampX, int ampY, double Ds, double Df, double CL, double CR,
                                    double rtol, int64_t max_iter, int64_t check_every, deff_next_image_fn next,
                                    deff_cg_image_done_fn done, void *user)
try {
    if (!c || !next || !done) return fail(DEFF_EINVAL, "NULL argument");
    if (!(rtol >= 0.0) || !std::isfinite(rtol)) return fail(DEFF_EINVAL, "deff_solve_cg_stream: rtol must be finite and >= 0");
    if (max_iter < 0) return fail(DEFF_EINVAL, "deff_solve_cg_stream: negative max_iter");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    if (c->slab)
        return fail(DEFF_EINVAL, "deff_solve_cg_stream: not for row-slab contexts (one image over row slabs: "
                                 "deff_slab_group_solve_cg or deff_slab_rank_solve_cg)");
    TRY(use_device(c));
    TRY(resident_check(c));                                          // an unchecked resident interval is settled under the OLD system
    // the table first, as a candidate of its own: a refusal (an inadmissible row, an image that does not match the mesh) leaves
    // every field of the context as it was -- its dictionary, a native 3-phase system, a caller's wall-column links
    std::vector<double> tab;
    {
        std::vector<double> rows;
        native2_rows(c, Ds, Df, CL, CR, rows);
        TRY(cg_table(rows, LUT_NATIVE_ROWS, tab));
        TRY(image_shape(c, W, H, ampX, ampY));
        commit_lut_rows(c, rows);
    }
    TRY(ensure_walls(c));
    TRY(dev_alloc(&c->code, c->n));
    TRY(dev_alloc(&c->q, (size_t)2 * c->nimg));
    const int B = c->nimg;
    const size_t npix = (size_t)W * H;
    c->CL = CL; c->CR = CR; c->Ds = Ds; c->Df = Df;
    c->phase_mode = 2; c->phase_D[0] = Df; c->phase_D[1] = Ds; c->phase_D[2] = 0.0;
    c->have_image = true; c->have_walls = true; c->have_matfree = true; c->have_explicit = false;
    c->links_sym = 0;
    dict_reset(c); c->have_field = true;
    adjoint_reset(c);
    c->q_valid = false;
    reset_batch_state(c);                                            // every slot's field lives in x[cur], now and afterwards
    double *x = c->x[c->cur];
    HIP_TRY(hipMemsetAsync(c->code, 0, sizeof(uint16_t) * c->n, c->stream));      // empty slots: zero rows, as deff_solve_stream
    HIP_TRY(hipMemsetAsync(c->x[0], 0, sizeof(double) * c->n, c->stream));
    HIP_TRY(hipMemsetAsync(c->x[1], 0, sizeof(double) * c->n, c->stream));
    HIP_TRY(hipMemsetAsync(c->Dl, 0, sizeof(double) * c->rows, c->stream));
    HIP_TRY(hipMemsetAsync(c->Dr, 0, sizeof(double) * c->rows, c->stream));
    HIP_TRY(hipMemsetAsync(c->pix, 0, npix * B, c->stream));

    CgGeom g = cg_geometry(c);
    const size_t items = (size_t)g.per_img * B;
    c->cg_plan_kr = g.kr;
    c->cg_plan_ntx = g.ntx;
    c->cg_plan_items = (int)g.per_img;
    c->cg_plan_restarts = 0;
    const bool onchip = c->cg_onchip && (size_t)c->nx * c->ny <= (size_t)CGI_CELLS;
    c->cg_plan_impl = onchip ? 2 : 1;
    const int fold = onchip ? 0 : c->cg_fold;
    c->cg_plan_fold = fold;
    if (onchip && !c->cg_cus) HIP_TRY(hipDeviceGetAttribute(&c->cg_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    TRY(cg_buffers(c, items));
    CgsBuffers bf;
    TRY(cgs_buffers(c, npix, &bf));
    int64_t launches = 0, waits = 0, intervals = 0;
    c->cgs_intervals = c->cgs_launches = c->cgs_waits = 0;
    auto figures = [&] {
        c->cgs_intervals = (int)std::min<int64_t>(intervals, INT32_MAX);
        c->cgs_launches = (int)std::min<int64_t>(launches, INT32_MAX);
        c->cgs_waits = (int)std::min<int64_t>(waits, INT32_MAX);
    };
    // whatever way the call ends, nothing of it is left in flight (the pinned buffers and `tab` are read by queued copies)
    struct Leave {
        deff_ctx *c;
        ~Leave() { (void)hipStreamSynchronize(c->stream); c->in_stream = false; }
    } leave{c};
    c->in_stream = true;                                             // deff_get_slot_field / deff_residual_slot: buf_of[] is current

    CgScal *sc = (CgScal *)c->cg_scal;
    // every slot parked (done = 4: no image) until an entry check starts it
    for (int k = 0; k < B; ++k) { bf.h_snap[0][k] = CgScal(); bf.h_snap[0][k].done = 4; }
    HIP_TRY(hipMemcpyAsync(sc, bf.h_snap[0], sizeof(CgScal) * B, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(bf.d_rounds, 0, sizeof(int) * B, c->stream));
    HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
    HIP_TRY(hipMemsetAsync(c->cg_tick, 0, sizeof(unsigned) * 2 * cgf_ticks(g.per_img, (size_t)B), c->stream));
    HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), sizeof(double) * CG_DOUBLES, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                        // h_snap[0] is a snapshot buffer from here on
    ++waits;

    const double tol2 = rtol * rtol;
    const dim3 grid((unsigned)((items + 3) / 4)), fin((unsigned)B);
    double *part = c->cg_part;
    const CgIteration iteration{c, false, fold, grid, fin, g, x, part, part + items, part + 2 * items, c->cg_tick,
                                c->cg_tick + cgf_ticks(g.per_img, (size_t)B), tol2, (long long)max_iter};
    struct Slot { bool live = false; int64_t id = -1, valid_from = 0; };
    std::vector<Slot> S(B);
    bool more = true;
    int n_live = 0;
    int64_t k_it = 0;                                                // streaming iterations enqueued (parity of the p buffers)

    // r = b - A x and the check of `n` listed slots (the list is on the device)
    auto resid_check = [&](const int *d_list, int n, int mode) -> int {
        CgGeom gl = g;
        gl.nimg = n;
        hipLaunchKernelGGL(k_cgs_resid, dim3((unsigned)(((size_t)g.per_img * n + 3) / 4)), dim3(256), 0, c->stream, c->cg_tab,
                           c->lut_nrows, c->code, x, c->cg_r, gl, d_list, part);
        hipLaunchKernelGGL(k_cgs_check, dim3((unsigned)n), dim3(CG_FIN), 0, c->stream, part, g.per_img, sc, d_list, bf.d_rounds,
                           tol2, (long long)max_iter, mode, CG_MAX_RESTARTS);
        HIP_TRY(hipGetLastError());
        launches += 2;
        return DEFF_OK;
    };
    // every free slot takes the next image: pixels and list go up in ONE copy, the slots rejoin at interval `from`
    auto enter = [&](int64_t from) -> int {
        int n = 0;
        for (int k = 0; k < B && more; ++k) {
            if (S[k].live) continue;
            int64_t id = -1;
            const int got = next(user, k, bf.h_pix + (size_t)n * npix, &id);
            if (got < 0) return fail(DEFF_EINVAL, "image source reported an error");
            if (got == 0) { more = false; break; }
            bf.h_new[n++] = k;
            S[k].live = true; S[k].id = id; S[k].valid_from = from;
            ++n_live;
        }
        if (!n) return DEFF_OK;
        HIP_TRY(hipMemcpyAsync(bf.d_new, bf.h_new, sizeof(int) * B + (size_t)n * npix, hipMemcpyHostToDevice, c->stream));
        const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(64, (c->n_img + 1023) / 1024));
        hipLaunchKernelGGL(k_cgs_enter, dim3(gx, (unsigned)n), dim3(256), 0, c->stream, bf.d_pix, bf.d_new, W, H, ampX, ampY,
                           c->nx, c->nxt, c->ny, Df, Ds, CL, CR, c->fma, c->pix, c->code, c->Dl, c->Dr, x);
        hipLaunchKernelGGL(k_cgs_admissible, dim3(gx, (unsigned)n), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code,
                           c->nx, c->ny, bf.d_new, c->cg_flags);
        HIP_TRY(hipGetLastError());
        launches += 2;
        return resid_check(bf.d_new, n, 0);
    };
    // the iteration work of one interval, then the slots' states on their way to the host
    auto interval = [&](int64_t i) -> int {
        if (onchip) {
            hipLaunchKernelGGL(k_cg_image, dim3((unsigned)std::min(B, c->cg_cus)), dim3(CGI_THREADS), 0, c->stream, c->cg_tab,
                               c->lut_nrows, c->code, x, c->cg_r, c->cg_p[0], sc, c->nx, c->ny, B, (long long)check_every, tol2,
                               (long long)max_iter);
            launches += 1;
        } else {
            for (int64_t q = 0; q < check_every; ++q, ++k_it)
                launches += iteration.enqueue(c->cg_p[k_it & 1], c->cg_p[(k_it + 1) & 1]);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bf.h_snap[i & 1], sc, sizeof(CgScal) * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(bf.h_flags[i & 1], c->cg_flags, sizeof(unsigned) * 2, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->cgs_ev[i & 1], c->stream));
        return DEFF_OK;
    };

    HIP_TRY(hipEventRecord(c->cg_ev0, c->stream));
    TRY(enter(0));
    if (n_live > 0) TRY(interval(0));
    for (int64_t i = 0; n_live > 0; ++i) {
        TRY(interval(i + 1));                                        // the GPU's next work, before the host handles interval i
        HIP_TRY(hipEventSynchronize(c->cgs_ev[i & 1]));
        ++waits;
        ++intervals;
        figures();
        if (bf.h_flags[i & 1][0])
            return fail(DEFF_EINVAL, "deff_solve_cg_stream: the system of an image is not symmetric (a link between two active "
                                     "cells differs from its partner, or an active row links out of its image)");
        int n_fin = 0;
        for (int k = 0; k < B; ++k)
            if (S[k].live && i >= S[k].valid_from && bf.h_snap[i & 1][k].done != 0) bf.h_fin[n_fin++] = k;
        if (!n_fin) continue;
        // the stopped slots' true residual (an image that misses rtol goes on), their fluxes, and both back in one wait
        HIP_TRY(hipMemcpyAsync(bf.d_fin, bf.h_fin, sizeof(int) * n_fin, hipMemcpyHostToDevice, c->stream));
        TRY(resid_check(bf.d_fin, n_fin, 1));
        hipLaunchKernelGGL(k_cgs_flux, dim3((unsigned)n_fin), dim3(256), 0, c->stream, x, c->Dl, c->Dr, c->nx, c->nxt, c->ny,
                           c->rows, c->dx, CL, CR, bf.d_fin, c->flux_reduce == 2 ? 1 : 0, c->mf, c->q);
        HIP_TRY(hipGetLastError());
        launches += 1;
        HIP_TRY(hipMemcpyAsync(bf.h_round, sc, sizeof(CgScal) * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(bf.h_q, c->q, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->cg_ev1, c->stream));
        HIP_TRY(hipEventSynchronize(c->cg_ev1));
        ++waits;
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->cg_ev0, c->cg_ev1));
        for (int q = 0; q < n_fin; ++q) {
            const int k = bf.h_fin[q];
            const CgScal &s = bf.h_round[k];
            if (s.done == 0) {                                       // restarted: back in the iteration from interval i + 2
                S[k].valid_from = i + 2;
                ++c->cg_plan_restarts;
                continue;
            }
            deff_cg_result res;
            res.iters = s.iters;
            res.rel_residual = s.rel;
            const double qAvg = (bf.h_q[2 * k] + bf.h_q[2 * k + 1]) / (2.0 * c->ny);      // deff_flux's expressions
            res.deff_raw = qAvg / ((CR - CL));
            res.loop_ms = ms;
            res.converged = s.rel <= rtol;
            S[k].live = false;
            --n_live;
            done(user, S[k].id, k, &res);                            // the slot's field is readable (deff_get_slot_field)
        }
        TRY(enter(i + 2));
        figures();
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                        // the interval enqueued ahead found every slot stopped
    ++waits;
    figures();
    return DEFF_OK;
}
DEFF_API_CATCH

// ---- conjugate gradients over row slabs: the steps of one slab (cg_slab.hpp; the loop is slab_solve_cg, api_slab.hip) -----

static_assert(SLCG_SLOT == CG_SLAB_SLOT, "gather slot width");

static CgSlabGeom slcg_geom(const CgSlab &s)
{
    const deff_ctx *c = s.c;
    return CgSlabGeom{c->nx, s.ntx, s.kr, c->own_lo, c->own_h, s.m_lo, s.m_hi, s.items};
}

// what deff_solve_cg asks of a context, for one slab; the table on success
static int slcg_admit(deff_ctx *c, std::vector<double> &tab)
{
    if (!c->have_field) return fail(DEFF_ESTATE, "no field: call init_linear or set_field on the slabs");
    if (!c->have_walls) return fail(DEFF_ESTATE, "wall diffusivities unknown (needed for Deff)");
    if (c->wrap_links)
        return fail(DEFF_EINVAL, "CG over row slabs: the system links a wall column to the neighbouring row (explicit-only system)");
    if (!c->have_matfree && c->have_explicit) TRY(ensure_dictionary(c));
    if (!c->have_matfree)
        return fail(DEFF_EINVAL, "CG over row slabs: the slab's system has no row dictionary (too many distinct rows, or "
                                 "dictionaries disabled): CG runs on the matrix-free form only");
    return cg_table(c, tab);
}

int slcg_setup(CgSlab *s, double rtol, int64_t max_iter)
{
    deff_ctx *c = s->c;
    TRY(use_device(c));
    s->refusal.clear();
    s->status = DEFF_OK;
    std::vector<double> tab;
    int rc = slcg_admit(c, tab);
    // geometry: kr and the strips from the whole image, the items from this slab's owned rows
    s->ntx = (c->nx + CG_COLS - 1) / CG_COLS;
    s->kr = cg_rows_per_item(s->ntx, c->mesh_ny);
    s->items = (unsigned)((size_t)s->ntx * ((c->own_h + s->kr - 1) / s->kr));
    s->m_lo = std::max(0, c->dom_lo);
    s->m_hi = std::min(c->rows, c->dom_lo + c->mesh_ny);
    s->tol2 = rtol * rtol;
    s->max_iter = (long long)max_iter;
    s->k = 0;
    // the work vectors only once the host's checks have passed (the check on the device needs the table and the flags there)
    if (rc == DEFF_OK) rc = cg_buffers(c, s->items);
    if (rc == DEFF_EHIP) return rc;
    if (rc != DEFF_OK) { s->refusal = g_err; s->status = rc; }
    if (rc == DEFF_OK) {
        HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
        // pageable source: the copy has left `tab` when the call returns
        HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), sizeof(double) * CG_DOUBLES, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        hipLaunchKernelGGL(k_slcg_admissible, dim3(grid_for((size_t)c->nx * (s->m_hi - s->m_lo), 2048)), dim3(256), 0, c->stream,
                           c->cg_tab, c->lut_nrows, c->code, c->nx, s->m_lo, s->m_hi, c->dom_lo >= 0 ? 1 : 0,
                           c->dom_lo + c->mesh_ny <= c->rows ? 1 : 0, c->cg_flags);
    }
    // the host's verdict travels as 1 - status (>= 2; 0 and 1 are the device's): the flags are not read then, and may not exist
    static_assert(DEFF_OK == 0 && DEFF_EINVAL < 0 && DEFF_ESTATE < 0 && DEFF_ENOMEM < 0, "verdict encoding");
    hipLaunchKernelGGL(k_slcg_verdict, dim3(1), dim3(1), 0, c->stream, c->cg_flags, rc == DEFF_OK ? 0.0 : (double)(1 - rc),
                       slcg_slot(*s, 2, s->me));
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

void slcg_commit(CgSlab *s)
{
    deff_ctx *c = s->c;
    c->cg_plan_kr = s->kr;
    c->cg_plan_ntx = s->ntx;
    c->cg_plan_items = (int)s->items;
    c->cg_plan_restarts = 0;
    c->cg_plan_impl = 1;
    c->cg_plan_fold = 0;                                             // row slabs: the gathers are a reduction of their own
}

int slcg_dir(CgSlab *s)
{
    deff_ctx *c = s->c;
    const CgSlabGeom g = slcg_geom(*s);
    double *p_in = c->cg_p[s->k & 1], *p_out = c->cg_p[(s->k + 1) & 1];
    hipLaunchKernelGGL(k_slcg_dir, dim3((g.items + 3) / 4), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, c->cg_r, p_in,
                       p_out, (const CgScal *)c->cg_scal, g, c->cg_part);
    if (s->nslabs > 1)
        hipLaunchKernelGGL(k_slcg_sum, dim3(1), dim3(CG_FIN), 0, c->stream, c->cg_part, g.items, 1, (size_t)0, 1,
                           slcg_slot(*s, 0, s->me));
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

int slcg_alpha_update(CgSlab *s)
{
    deff_ctx *c = s->c;
    const CgSlabGeom g = slcg_geom(*s);
    double *p = c->cg_p[(s->k + 1) & 1];
    double *part_rz = c->cg_part + g.items, *part_rr = c->cg_part + 2 * (size_t)g.items;
    hipLaunchKernelGGL(k_slcg_alpha, dim3(1), dim3(CG_FIN), 0, c->stream, c->cg_part, g.items, slcg_slot(*s, 0, 0), s->nslabs, s->me,
                       (CgScal *)c->cg_scal);
    hipLaunchKernelGGL(k_slcg_update, dim3((g.items + 3) / 4), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, p,
                       c->x[c->cur], c->cg_r, (const CgScal *)c->cg_scal, g, part_rz, part_rr);
    if (s->nslabs > 1)
        hipLaunchKernelGGL(k_slcg_sum, dim3(1), dim3(CG_FIN), 0, c->stream, part_rz, g.items, 1, (size_t)g.items, 2,
                           slcg_slot(*s, 1, s->me));
    HIP_TRY(hipGetLastError());
    ++s->k;
    return DEFF_OK;
}

int slcg_beta(CgSlab *s)
{
    deff_ctx *c = s->c;
    double *part_rz = c->cg_part + s->items, *part_rr = c->cg_part + 2 * (size_t)s->items;
    hipLaunchKernelGGL(k_slcg_beta, dim3(1), dim3(CG_FIN), 0, c->stream, part_rz, part_rr, s->items, slcg_slot(*s, 1, 0), s->nslabs,
                       s->me, (CgScal *)c->cg_scal, s->tol2, s->max_iter);
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

int slcg_resid(CgSlab *s)
{
    deff_ctx *c = s->c;
    const CgSlabGeom g = slcg_geom(*s);
    hipLaunchKernelGGL(k_slcg_resid, dim3((g.items + 3) / 4), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, c->x[c->cur],
                       c->cg_r, g, c->cg_part);
    if (s->nslabs > 1)
        hipLaunchKernelGGL(k_slcg_sum, dim3(1), dim3(CG_FIN), 0, c->stream, c->cg_part, g.items, 3, (size_t)1, 3,
                           slcg_slot(*s, 2, s->me));
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

int slcg_check(CgSlab *s, int mode, int allow_restart)
{
    deff_ctx *c = s->c;
    if (mode == 1) HIP_TRY(hipMemsetAsync(c->cg_flags + 1, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_slcg_check, dim3(1), dim3(CG_FIN), 0, c->stream, c->cg_part, s->items, slcg_slot(*s, 2, 0), s->nslabs, s->me,
                       (CgScal *)c->cg_scal, s->tol2, s->max_iter, mode, allow_restart, c->cg_flags + 1);
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

int slcg_read(CgSlab *s, CgSlabState *out)
{
    deff_ctx *c = s->c;
    CgScal h;
    unsigned flag = 0;
    HIP_TRY(hipMemcpyAsync(&h, c->cg_scal, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&flag, c->cg_flags + 1, sizeof flag, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = CgSlabState{h.iters, h.rel, h.done, flag};
    return DEFF_OK;
}
