// api_cg.hip -- deff_solve_cg: Jacobi-preconditioned conjugate gradients to a residual tolerance (kernels_cg.hpp).  Not the
// reference's algorithm: it reaches the same discrete fixed point (same A, b, wall-flux Deff) as the weighted Jacobi loop of
// deff_solve, in far fewer iterations.  Nothing of the Jacobi path is touched: its tables (lut, c0 plane), plans and knobs
// stay as they are (the "fma" knob does not apply here: CG's arithmetic is written-order FP64 only).
#include "ctx.hpp"
#include "kernels_cg.hpp"
#include "kernels_cg_image.hpp"
#include <vector>

// true-residual rounds that may restart the recurrence of a finished image (each round costs one pass and a synchronisation)
static constexpr int CG_MAX_RESTARTS = 8;

// CG table from the host dictionary: planes A0, 1/A0, aW, aE, aS, aN, b; decoupled rows (four zero links, b == 0) stay all
// zeros.  An active row must have a finite positive A0 with a normal 1/A0 and finite links and b.
static int cg_table(const deff_ctx *c, std::vector<double> &t)
{
    t.assign(CG_DOUBLES, 0.0);
    constexpr int S = LUT_PLANE_STRIDE;
    for (int k = 1; k < c->lut_nrows; ++k) {
        const double *row = &c->lut_rows[(size_t)k * 6];
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

// Work items of one image: strips of 128 columns x kr rows, kr chosen from (nx, ny) alone so that an image of a stack is cut
// (and its sums ordered) exactly like a one-image context's; ~8 192 items per image, 2..16 rows each.
static CgGeom cg_geometry(const deff_ctx *c)
{
    CgGeom g;
    g.nx = c->nx;
    g.ny = c->ny;
    g.nimg = c->nimg;
    g.ntx = (c->nx + CG_COLS - 1) / CG_COLS;
    const long want = (long)g.ntx * c->ny / 8192;
    g.kr = (int)std::max(2L, std::min(16L, want));
    g.cpi = (c->ny + g.kr - 1) / g.kr;
    g.per_img = (unsigned)((size_t)g.ntx * g.cpi);
    return g;
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
        return fail(DEFF_EINVAL, "deff_solve_cg: not for row-slab contexts (CG over row slabs needs an all-reduce per iteration)");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field: call deff_init_linear() or deff_set_field()");
    if (!c->have_walls) return fail(DEFF_ESTATE, "wall diffusivities unknown (needed for Deff)");
    if (c->wrap_links)
        return fail(DEFF_EINVAL, "deff_solve_cg: the system links a wall column to the neighbouring row (explicit-only system)");
    TRY(use_device(c));
    TRY(consolidate(c));                                             // every image's newest field in x[cur]
    if (!c->have_matfree && c->have_explicit) TRY(ensure_dictionary(c));
    if (!c->have_matfree)
        return fail(DEFF_EINVAL, "deff_solve_cg: the system has no row dictionary (too many distinct rows, or dictionaries "
                                 "disabled): CG runs on the matrix-free form only");
    std::vector<double> tab;
    TRY(cg_table(c, tab));
    const CgGeom g = cg_geometry(c);
    const size_t items = (size_t)g.per_img * c->nimg;
    c->cg_plan_kr = g.kr;
    c->cg_plan_ntx = g.ntx;
    c->cg_plan_items = (int)g.per_img;
    c->cg_plan_restarts = 0;
    // on chip (tuning "cg_onchip"): an image whose arrays fit one compute unit's LDS and registers iterates there, one
    // launch per check_every iterations instead of four per iteration; larger images keep the streaming kernels
    const bool onchip = c->cg_onchip && (size_t)c->nx * c->ny <= (size_t)CGI_CELLS;
    c->cg_plan_impl = onchip ? 2 : 1;
    if (onchip && !c->cg_cus) HIP_TRY(hipDeviceGetAttribute(&c->cg_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    TRY(cg_buffers(c, items));
    HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), sizeof(double) * CG_DOUBLES, hipMemcpyHostToDevice, c->stream));

    // admissibility: active links symmetric bit for bit, no link out of the image; nothing is changed on a refusal
    unsigned flags[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(c->cg_flags, 0, sizeof(unsigned) * 2, c->stream));
    hipLaunchKernelGGL(k_cg_admissible, dim3(grid_for(c->n, 2048)), dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code,
                       c->nx, c->rows, c->ny, c->cg_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags, c->cg_flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[0])
        return fail(DEFF_EINVAL, "deff_solve_cg: the system is not symmetric (a link between two active cells differs from "
                                 "its partner, or an active row links out of its image)");

    const double tol2 = rtol * rtol;
    const dim3 grid((unsigned)((items + 3) / 4)), fin((unsigned)c->nimg);
    double *x = c->x[c->cur];
    double *part = c->cg_part, *part_rz = c->cg_part + items, *part_rr = c->cg_part + 2 * items;
    CgScal *sc = (CgScal *)c->cg_scal;
    std::vector<CgScal> hs(c->nimg);
    auto true_residual = [&](int mode, int allow) -> int {
        hipLaunchKernelGGL(k_cg_resid, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, x, c->cg_r, g, part);
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
            HIP_TRY(hipMemcpyAsync(&flags[1], c->cg_flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(hs.data(), sc, sizeof(CgScal) * c->nimg, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (flags[1] == 0) break;
            ++rounds;
            c->cg_plan_restarts = rounds;
        }
        if (onchip) {
            // up to check_every iterations of every running image, p in cg_p[0] throughout (the streaming loop below starts
            // every call at cg_p[0] with the restart flag set, so the two forms never read each other's p)
            hipLaunchKernelGGL(k_cg_image, dim3((unsigned)std::min(c->nimg, c->cg_cus)), dim3(CGI_THREADS), 0, c->stream,
                               c->cg_tab, c->lut_nrows, c->code, x, c->cg_r, c->cg_p[0], sc, c->nx, c->ny, c->nimg,
                               (long long)check_every, tol2, (long long)max_iter);
            HIP_TRY(hipGetLastError());
            continue;
        }
        for (int64_t i = 0; i < check_every; ++i, ++k) {
            double *p_in = c->cg_p[k & 1], *p_out = c->cg_p[(k + 1) & 1];
            hipLaunchKernelGGL(k_cg_dir, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, c->cg_r, p_in, p_out,
                               sc, g, part);
            hipLaunchKernelGGL(k_cg_alpha, fin, dim3(CG_FIN), 0, c->stream, part, g.per_img, sc);
            hipLaunchKernelGGL(k_cg_update, grid, dim3(256), 0, c->stream, c->cg_tab, c->lut_nrows, c->code, p_out, x, c->cg_r,
                               sc, g, part_rz, part_rr);
            hipLaunchKernelGGL(k_cg_beta, fin, dim3(CG_FIN), 0, c->stream, part_rz, part_rr, g.per_img, sc, tol2,
                               (long long)max_iter);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->cg_ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->cg_ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->cg_ev0, c->cg_ev1));

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
