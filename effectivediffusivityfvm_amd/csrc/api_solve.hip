// api_solve.hip -- the wall fluxes and the Jacobi solve loops of libdeff_amd.so: the host side of
// JacobiGPU (Deff2DGPU/Deff2D.cuh:1163-1314) for one image, a stack of images and a stream of
// images through a stack.  The loops ask api_sweep.hip for a plan and hand it back with a sweep count; no sweep kernel
// is compiled here.  See ctx.hpp for the file map, DESIGN.md section 4-6 for the design.
#include "ctx.hpp"

// Wall fluxes of the current field (cuh:1256-1257) for every stacked row, brought to the
// pinned host buffer: mf_host[0..rows) left wall, mf_host[rows..2*rows) right wall.
int flux_rows(deff_ctx *c, bool need_rows)
{
    if (!c->have_walls)
        return fail(DEFF_ESTATE, "wall diffusivities unknown: pass D to deff_set_system() or assemble on the device");
    TRY(resident_check(c));
    hipLaunchKernelGGL(k_wall_flux, dim3((c->rows + 255) / 256), dim3(256), 0, c->stream, c->x[c->cur], c->Dl,
                       c->Dr, c->nx, c->nxt, c->rows, c->dx, c->CL, c->CR, c->mf);
    HIP_TRY(hipGetLastError());
    c->q_valid = false;
    if (c->flux_reduce && !c->slab) {
        // sums on the device (kernels_setup.hpp: k_flux_sum): the check moves 16 B per image
        TRY(dev_alloc(&c->q, (size_t)2 * c->nimg));
        if (!c->q_host) HIP_TRY(hipHostMalloc((void **)&c->q_host, sizeof(double) * 2 * c->nimg));
        const dim3 grid((c->nimg + 3) / 4);
        if (c->flux_reduce == 2) hipLaunchKernelGGL(k_flux_sum<true>, grid, dim3(256), 0, c->stream, c->mf, c->rows, c->ny, c->nimg, c->q);
        else hipLaunchKernelGGL(k_flux_sum<false>, grid, dim3(256), 0, c->stream, c->mf, c->rows, c->ny, c->nimg, c->q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->q_host, c->q, sizeof(double) * 2 * c->nimg, hipMemcpyDeviceToHost, c->stream));
        c->q_valid = true;
        if (!need_rows) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            return dealt_watch(c);
        }
    }
    HIP_TRY(hipMemcpyAsync(c->mf_host, c->mf, sizeof(double) * 2 * c->rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return dealt_watch(c);
}

// Deff of image k from its wall fluxes, summed in row order like the reference (cuh:1258-1263): on the host from
// mf_host, or from the device's sums when flux_rows() produced them.
static double deff_of_image(const deff_ctx *c, int k)
{
    if (!c->q_valid)
        return deff_of_fluxes(c->mf_host + (size_t)k * c->ny, c->mf_host + c->rows + (size_t)k * c->ny, c->ny, c->CL, c->CR);
    const double Q1 = c->q_host[2 * k], Q2 = c->q_host[2 * k + 1];
    const double qAvg = (Q1 + Q2) / (2.0 * c->ny);
    return qAvg / ((c->CR - c->CL));
}

static void copy_fluxes(const deff_ctx *c, double *MFL, double *MFR)
{
    if (MFL) memcpy(MFL, c->mf_host, sizeof(double) * c->rows);
    if (MFR) memcpy(MFR, c->mf_host + c->rows, sizeof(double) * c->rows);
}

// deff_raw: nimg values (one per stacked image); MFL/MFR: rows values each, may be NULL.
extern "C" int deff_flux(deff_ctx *c, double *deff_raw, double *MFL, double *MFR)
try {
    if (!c || !deff_raw) return fail(DEFF_EINVAL, "NULL argument");
    if (!c->have_field) return fail(DEFF_ESTATE, "no field");
    TRY(use_device(c));
    TRY(consolidate(c));
    TRY(flux_rows(c, MFL || MFR));
    for (int k = 0; k < c->nimg; ++k) deff_raw[k] = deff_of_image(c, k);
    copy_fluxes(c, MFL, MFR);
    return DEFF_OK;
}
DEFF_API_CATCH

// JacobiGPU's loop, cuh:1232-1290, with the sweeps between two checks enqueued without host
// round trips.  `iter` counts completed sweeps; the sweep with 0-based index k is followed by a
// check iff k % check_every == 0 (cuh:1243).  All images of a batch start together, so their
// checks coincide; each image carries its own JacobiCheck and drops out (is frozen in the
// buffer it is in) as soon as ITS stopping rule fires -- exactly what a one-image-at-a-time run
// of the reference's loop would do.
extern "C" int deff_solve_batch(deff_ctx *c, double omega, double tol, int64_t max_iter, int64_t check_every,
                                deff_result *out, double *MFL, double *MFR)
try {
    if (!c || !out) return fail(DEFF_EINVAL, "NULL argument");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    TRY(use_device(c));
    SweepPlan pl;
    TRY(plan_sweeps(c, omega, &pl));
    if (!c->have_walls) return fail(DEFF_ESTATE, "wall diffusivities unknown (needed for Deff)");
    TRY(consolidate(c));                                             // x is in/out: warm start from x[cur]
    reset_batch_state(c);                                            // every image iterates again

    const int B = c->nimg;
    std::vector<JacobiCheck> chk(B);
    std::vector<int64_t> iters(B, 0);
    int n_active = (max_iter > 0 && JacobiCheck().more(tol)) ? B : 0;   // cuh:1232 before the first check
    if (n_active == 0) c->active_h.assign(B, 0);
    int64_t iter = 0;
    c->last_launches = 0;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    while (iter < max_iter && n_active > 0) {                        // cuh:1232
        const CheckStep st = check_step(iter, max_iter, check_every);
        TRY(enqueue_sweeps(c, pl, st.sweeps));
        iter += st.sweeps;
        for (int k = 0; k < B; ++k)
            if (c->active_h[k]) { iters[k] = iter; c->buf_of[k] = (uint8_t)c->cur; }
        if (st.check) {
            TRY(flux_rows(c, MFL || MFR));
            bool froze = false;
            for (int k = 0; k < B; ++k) {
                if (!c->active_h[k]) continue;
                chk[k].update(deff_of_image(c, k));
                if (B == 1 && c->progress) c->progress(st.next_check, chk[k].deffNew, chk[k].change, c->progress_user);
                if (!chk[k].more(tol)) { c->active_h[k] = 0; --n_active; froze = true; }
            }
            if (B == 1) copy_fluxes(c, MFL, MFR);
            else {
                // keep, per image, the fluxes of ITS last check
                for (int k = 0; k < B; ++k)
                    if (chk[k].checks && iters[k] == iter) {
                        if (MFL) memcpy(MFL + (size_t)k * c->ny, c->mf_host + (size_t)k * c->ny, sizeof(double) * c->ny);
                        if (MFR) memcpy(MFR + (size_t)k * c->ny, c->mf_host + c->rows + (size_t)k * c->ny,
                                        sizeof(double) * c->ny);
                    }
            }
            if (froze && n_active > 0) {
                TRY(dev_alloc(&c->active, (size_t)B));
                HIP_TRY(hipMemcpyAsync(c->active, c->active_h.data(), (size_t)B, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                c->masked = true;
            }
        }
    }
    TRY(resident_check(c));                                          // a solve that ends between two checks (MAX_ITER)
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    for (int k = 0; k < B; ++k) out[k] = chk[k].result(iters[k], ms);     // the batch shares one loop (loop_ms)
    return DEFF_OK;
}
DEFF_API_CATCH

// ---- streaming batch ---------------------------------------------------------------------
//
// Dataset generation with images that converge after very different numbers of sweeps: a plain
// batch drains (its slots empty one by one, measured 376 of ~1000 G cells*iter/s end to end on 512
// images of 128^2).  Here a slot whose image has finished is REFILLED with the next image.  To keep
// every image on the reference's schedule -- checks after its own sweeps 1, C+1, 2C+1, ... -- new
// images enter exactly one sweep before a check of the running ones: that sweep is their sweep 1,
// so all slots share the check points for ever.  Per image the arithmetic and the stopping rule are
// those of a one-image run (cuh:1232-1290).

// put image `slot`'s pixels / codes / wall data / linear guess in place (2-phase native system)
static int stream_load_slot(deff_ctx *c, int slot, const uint8_t *pix_host)
{
    TRY(resident_check(c));                            // the restart copy of a resident interval predates this slot's new image
    const size_t npix = (size_t)c->W * c->H;
    uint8_t *dpix = c->pix + (size_t)slot * npix;
    uint16_t *dcode = c->code + (size_t)slot * c->n_img;
    HIP_TRY(hipMemcpyAsync(dpix, pix_host, npix, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));        // pix_host is the caller's scratch
    hipLaunchKernelGGL(k_phase_codes, dim3(grid_for(c->n_img)), dim3(256), 0, c->stream, dpix, c->W, c->ampX, c->ampY,
                       c->nx, c->nxt, c->ny, c->ny, 0, c->ny, dcode);
    hipLaunchKernelGGL(k_wall_D_2phase, dim3((c->ny + 255) / 256), dim3(256), 0, c->stream, dpix, c->W, c->ampX, c->ampY,
                       c->nxt, c->ny, c->ny, c->Df, c->Ds, c->Dl + (size_t)slot * c->ny, c->Dr + (size_t)slot * c->ny);
    hipLaunchKernelGGL(k_init_linear, dim3(grid_for(c->n_img)), dim3(256), 0, c->stream,
                       c->x[c->cur] + (size_t)slot * c->n_img, c->nx, c->nxt, c->ny, c->CL, c->CR, c->fma);
    HIP_TRY(hipGetLastError());
    c->buf_of[slot] = (uint8_t)c->cur;
    c->links_sym = 0;                                  // new codes in this slot
    c->have_explicit = false;                          // ... and coefficient planes, if any, that belong to the image before
    return DEFF_OK;
}

static int stream_push_mask(deff_ctx *c, int n_active)
{
    TRY(resident_check(c));                            // ... and the mask the interval ran under
    bool all = true;
    for (int k = 0; k < c->nimg; ++k) all = all && c->active_h[k];
    c->masked = !all && n_active > 0;
    if (c->masked) {
        TRY(dev_alloc(&c->active, (size_t)c->nimg));
        HIP_TRY(hipMemcpyAsync(c->active, c->active_h.data(), (size_t)c->nimg, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return DEFF_OK;
}

extern "C" int deff_get_slot_field(deff_ctx *c, int slot, double *x)
try {
    if (!c || !x || slot < 0 || slot >= c->nimg) return fail(DEFF_EINVAL, "bad slot");
    TRY(use_device(c));
    TRY(rows_d2h(c, x, (const double *)(c->x[(c->masked || c->in_stream) ? c->buf_of[slot] : c->cur] + (size_t)slot * c->n_img),
                 (size_t)c->ny));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_solve_stream(deff_ctx *c, int W, int H, int ampX, int ampY, double Ds, double Df, double CL,
                                 double CR, double omega, double tol, int64_t max_iter, int64_t check_every,
                                 deff_next_image_fn next, deff_image_done_fn done, void *user)
try {
    if (!c || !next || !done) return fail(DEFF_EINVAL, "NULL argument");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    if (c->slab) return fail(DEFF_EINVAL, "not for slab contexts");
    TRY(use_device(c));
    std::vector<double> rows;
    native2_rows(c, Ds, Df, CL, CR, rows);
    if (c->prescaled) {
        // what plan_sweeps would refuse below, with the images taken and the old system gone: said here, where a refusal still
        // leaves field, system and plan as they were (deff_amd.h, "prescaled")
        if (c->kernel == DEFF_KERNEL_EXPLICIT || c->kernel == DEFF_KERNEL_SCALAR)
            return fail(DEFF_EINVAL, "prescaled: the explicit and scalar kernels have no pre-scaled form (deff_set_kernel: auto, matfree or matfree_tb)");
        for (int k = 1; k < LUT_NATIVE_ROWS; ++k)
            if (!std::isfinite(omega / rows[(size_t)k * 6]))
                return fail(DEFF_EINVAL, "prescaled: the row dictionary has a singular row (a phase that cannot diffuse): "
                                         "omega / A0 is not finite there and the table cannot be pre-scaled");
    }
    TRY(image_shape(c, W, H, ampX, ampY));
    TRY(ensure_walls(c));
    TRY(dev_alloc(&c->code, c->n));
    const int B = c->nimg;
    c->CL = CL; c->CR = CR; c->Ds = Ds; c->Df = Df;
    c->phase_mode = 2; c->phase_D[0] = Df; c->phase_D[1] = Ds; c->phase_D[2] = 0.0;
    commit_lut_rows(c, rows);
    c->have_image = true; c->have_walls = true; c->have_matfree = true; c->have_explicit = false;
    c->links_sym = 0;
    dict_reset(c); c->have_field = true;
    adjoint_reset(c);
    HIP_TRY(hipMemsetAsync(c->code, 0, sizeof(uint16_t) * c->n, c->stream));      // empty slots: zero rows
    HIP_TRY(hipMemsetAsync(c->x[0], 0, sizeof(double) * c->n, c->stream));
    HIP_TRY(hipMemsetAsync(c->x[1], 0, sizeof(double) * c->n, c->stream));
    // ... and zero wall diffusivities and pixels, so that their Deff is 0 and not what the allocation held
    HIP_TRY(hipMemsetAsync(c->Dl, 0, sizeof(double) * c->rows, c->stream));
    HIP_TRY(hipMemsetAsync(c->Dr, 0, sizeof(double) * c->rows, c->stream));
    HIP_TRY(hipMemsetAsync(c->pix, 0, (size_t)W * H * B, c->stream));
    reset_batch_state(c);

    struct Slot { bool live = false; int64_t id = -1, iters = 0; JacobiCheck chk; };
    std::vector<Slot> S(B);
    std::vector<uint8_t> pixbuf((size_t)W * H);
    bool more = true;
    int n_active = 0;
    auto refill = [&]() -> int {                       // fill every free slot while images remain
        for (int k = 0; k < B && more; ++k) {
            if (S[k].live) continue;
            int64_t id = -1;
            const int got = next(user, k, pixbuf.data(), &id);
            if (got < 0) return fail(DEFF_EINVAL, "image source reported an error");
            if (got == 0) { more = false; break; }
            TRY(stream_load_slot(c, k, pixbuf.data()));
            S[k] = Slot();
            S[k].live = true; S[k].id = id;
            c->active_h[k] = 1;
            ++n_active;
        }
        return DEFF_OK;
    };
    auto retire = [&](int k, float ms) {
        const deff_result r = S[k].chk.result(S[k].iters, ms);
        c->active_h[k] = 0;
        --n_active;
        done(user, S[k].id, k, &r);                    // the slot's field is still readable (deff_get_slot_field)
        S[k].live = false;
    };
    auto advance = [&](SweepPlan &pl, int64_t nsw) -> int {
        if (nsw <= 0) return DEFF_OK;
        TRY(enqueue_sweeps(c, pl, nsw));
        for (int k = 0; k < B; ++k)
            if (S[k].live) { S[k].iters += nsw; c->buf_of[k] = (uint8_t)c->cur; }
        return DEFF_OK;
    };

    for (int k = 0; k < B; ++k) c->active_h[k] = 0;
    c->in_stream = true;
    struct Leave { deff_ctx *c; ~Leave() { c->in_stream = false; } } leave{c};
    TRY(refill());
    SweepPlan pl;
    TRY(plan_sweeps(c, omega, &pl));
    c->last_launches = 0;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    if (!(max_iter > 0 && JacobiCheck().more(tol))) {  // cuh:1232 before the first check: no sweep at all
        for (;;) {
            for (int k = 0; k < B; ++k) if (S[k].live) retire(k, 0.f);
            if (!more) break;
            TRY(refill());
            if (n_active == 0) break;
        }
    }
    // phase of max_iter inside a check interval: live images sit at iters = j*C + 1 after a check
    while (n_active > 0) {
        TRY(stream_push_mask(c, n_active));
        // one sweep (the first of the newly loaded images, sweep j*C + 1 of the others), then the check
        TRY(advance(pl, 1));
        TRY(flux_rows(c, false));                      // a stream reports no per-row fluxes
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(hipEventSynchronize(c->ev1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        for (int k = 0; k < B; ++k) {
            if (!S[k].live) continue;
            S[k].chk.update(deff_of_image(c, k));
            if (!S[k].chk.more(tol) || S[k].iters >= max_iter) retire(k, ms);
        }
        if (n_active == 0 && !more) break;
        // up to the next check: C - 1 sweeps, split where images run into max_iter (they all carry
        // iters = j*C + 1 with their own j, so each reaches max_iter the same distance after a check)
        int64_t left = check_every - 1;
        while (left > 0 && n_active > 0) {
            int64_t seg = left;
            for (int k = 0; k < B; ++k)
                if (S[k].live && max_iter - S[k].iters < seg) seg = max_iter - S[k].iters;
            if (seg > 0) {
                TRY(stream_push_mask(c, n_active));
                TRY(advance(pl, seg));
                left -= seg;
            }
            bool hit = false;
            for (int k = 0; k < B; ++k)
                if (S[k].live && S[k].iters >= max_iter) { hit = true; }
            if (hit) {
                TRY(resident_check(c));                // the retired images' fields are handed out now: settle the interval first
                HIP_TRY(hipEventRecord(c->ev1, c->stream));
                HIP_TRY(hipEventSynchronize(c->ev1));
                float ms2 = 0;
                HIP_TRY(hipEventElapsedTime(&ms2, c->ev0, c->ev1));
                for (int k = 0; k < B; ++k)
                    if (S[k].live && S[k].iters >= max_iter) retire(k, ms2);   // MAX_ITER reached between checks, cuh:1232
            }
        }
        TRY(refill());                                 // newcomers start with the sweep that precedes the next check
        TRY(replan_for_new_codes(c, omega, &pl));      // new images, new codes: what the plan took for granted is looked at again
    }
    // What the context holds from here on (deff_amd.h): slot k = the last image that ran in it, its system and its final
    // field.  A slot that retired while others kept sweeping is frozen in the buffer it stopped in, and that is x[cur] only
    // if the flips since then are even: bring every slot's newest field into x[cur] (consolidate() settles the last resident
    // interval first; it acts only under a mask, and the stream's last mask may already be gone) before buf_of is forgotten.
    c->masked = true;
    TRY(consolidate(c));
    reset_batch_state(c);
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_solve(deff_ctx *c, double omega, double tol, int64_t max_iter, int64_t check_every,
                          deff_result *out, double *MFL, double *MFR)
try {
    if (c && c->nimg != 1) return fail(DEFF_EINVAL, "context holds %d images: use deff_solve_batch()", c->nimg);
    return deff_solve_batch(c, omega, tol, max_iter, check_every, out, MFL, MFR);
}
DEFF_API_CATCH

extern "C" int deff_set_progress(deff_ctx *c, deff_progress_fn fn, void *user)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    c->progress = fn;
    c->progress_user = user;
    return DEFF_OK;
}
DEFF_API_CATCH
