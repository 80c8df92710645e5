// api_slab.hip -- one image over several GPUs as row slabs (BASELINE config #4).
// See ctx.hpp for the file map.
#include <rccl/rccl.h>

#include <functional>

#include "cg_slab.hpp"
#include "ctx.hpp"

// ====================================================================== row slabs ==
//
// One image split into N contiguous row slabs, one per GPU (BASELINE config #4).
// The reference has nothing like it (cudaSetDevice(0), cuh:908).  Each slab is an ordinary
// context whose arrays carry SLAB_HALO extra rows above and below its own rows; a temporally
// blocked pass of T <= SLAB_HALO sweeps needs exactly T valid halo rows, so ONE exchange per
// pass (not per sweep) refreshes them: every slab sends its first and last SLAB_HALO own rows
// to its neighbours.  No arithmetic changes, so the assembled field is bit-identical to the
// one-GPU field, and the wall fluxes are summed on the host in global row order, so Deff and the
// stopping decision are too.
//
// Two forms share the slabs, the pass loop and the solve loop below; they differ in the transport
// only.  The group drives all slabs from one host thread (one process, N devices; copies between
// devices are hipMemcpyPeerAsync over xGMI, ordered by events) -- which is also what lets the
// whole path be exercised with N slabs on a single GPU.  The rank is one slab per process: RCCL
// send/recv of the same row blocks + an all-gather of the fluxes, or a caller-supplied transport.

static const int SLAB_HALO = 8;

// The launch plans of one slab's pass: the whole slab in one launch, or -- so that the exchange can start while most of
// the slab is still being swept -- the two SLAB_HALO-row bands the neighbours wait for, then the interior.
struct SlabPass {
    SweepPlan whole, top, bot, mid;
    bool split = false;
};

// One slab of an image: its context, and for the overlap of the exchange with the interior of the pass a second stream
// for the exchange and two events -- bnd: "the rows my neighbours wait for (first / last SLAB_HALO owned rows) are
// written", halo: "my halo rows hold the neighbours' new rows".
struct Slab {
    deff_ctx *c = nullptr;
    int g0 = 0, own = 0;                      // first global row and row count
    hipStream_t xs = nullptr;
    hipEvent_t bnd = nullptr, halo = nullptr;
    SlabPass plT, pl1;                        // passes of T sweeps and of one sweep (slab_plans)
    // conjugate gradients (slab_solve_cg), made by the first one: the solve's state, the gathered sums on the device and
    // the event "this slab's rows and its gather slot are written"
    CgSlab cg;
    double *cg_all = nullptr;
    hipEvent_t cg_ev = nullptr;
};

// The slabs one call drives and how their halo rows travel: a group's N slabs with peer copies, or a rank's one slab
// with RCCL or the caller's transport.  exchange(r, xs) enqueues the exchange of slab r after a pass on xs, behind the
// `bnd` events of the rows it moves.
struct SlabSet {
    Slab *s;
    int n;
    int overlap;                              // slab_overlap as it applies to these slabs
    std::function<int(int r, hipStream_t xs)> exchange;
    // what conjugate gradients need beyond it (slab_solve_cg), each enqueued on slab r's stream behind the neighbours' cg_ev:
    int total = 1, first = 0;                 // slabs of the image, and which of them s[0] is
    // the row of buf(slab) next to each neighbour goes into that neighbour's adjacent halo row (and theirs into r's)
    std::function<int(int r, double *(*buf)(const Slab &))> send_row;
    std::function<int(int r, int phase)> gather;          // every slab's CG_SLAB_SLOT doubles of `phase` into every slab's cg_all
    std::function<int(int r)> settle;                     // r's stream waits until its neighbours have taken what `exchange` moves
};

// overlap: 0 = never split, 1 = split when it pays (a slab of >= 16 Mi cells: three launches + the stream hand-overs
// cost ~10 us of host time per pass, which a small slab does not have -- 4 slabs of 4096 x 1024 on one GPU: 226 us per
// pass split against 185 us unsplit, whereas 4 slabs of 16384 x 4096 hide the exchange completely), 2 = always
static int slab_pass_plans(deff_ctx *c, double omega, int T_override, int overlap, SlabPass *sp)
{
    sp->whole = SweepPlan();
    sp->whole.T_override = T_override;
    TRY(plan_sweeps(c, omega, &sp->whole));
    if (sp->whole.kernel != DEFF_KERNEL_MATFREE_TB) return fail(DEFF_ESTATE, "row-slab mode needs the temporally blocked kernel");
    // keyed on tb_ref_cells -- a figure of (nx, NY, slab count) alone -- so that every slab / rank of an image splits alike
    const size_t ref = c->tb_ref_cells ? c->tb_ref_cells : c->n;
    sp->split = (overlap == 2 || (overlap == 1 && ref >= ((size_t)1 << 24))) && c->own_h >= 3 * SLAB_HALO;
    if (!sp->split) return DEFF_OK;
    const int lo[3] = {c->own_lo, c->own_lo + c->own_h - SLAB_HALO, c->own_lo + SLAB_HALO};
    const int h[3] = {SLAB_HALO, SLAB_HALO, c->own_h - 2 * SLAB_HALO};
    SweepPlan *pl[3] = {&sp->top, &sp->bot, &sp->mid};
    for (int k = 0; k < 3; ++k) {
        *pl[k] = SweepPlan();
        pl[k]->T_override = sp->whole.T;       // the same sweeps per pass as the whole-slab plan
        pl[k]->band_lo = lo[k];
        pl[k]->band_h = h[k];
        TRY(plan_sweeps(c, omega, pl[k]));
        if (pl[k]->kernel != DEFF_KERNEL_MATFREE_TB) return fail(DEFF_ESTATE, "row-slab mode needs the temporally blocked kernel");
    }
    return DEFF_OK;
}

// Enqueue one pass of a slab on its stream: the bands first (then `bnd`), the interior behind them; flips x[cur].
static int slab_enqueue_pass(deff_ctx *c, const SlabPass &sp, hipEvent_t bnd)
{
    if (sp.split) {
        TRY(launch_tb_pass(c, sp.top));
        TRY(launch_tb_pass(c, sp.bot));
        HIP_TRY(hipEventRecord(bnd, c->stream));
        TRY(launch_tb_pass(c, sp.mid));
        c->last_launches += 3;
    } else {
        TRY(launch_tb_pass(c, sp.whole));
        HIP_TRY(hipEventRecord(bnd, c->stream));
        ++c->last_launches;
    }
    c->cur ^= 1;
    HIP_TRY(hipGetLastError());
    return DEFF_OK;
}

// first global row of slab r of n (slab r owns rows [slab_first(r), slab_first(r + 1)))
static int slab_first(int NY, int n, int r) { return (int)((long long)NY * r / n); }

static int slab_check(int nx, int NY, int n, const char *parts)
{
    if (nx < 2) return fail(DEFF_EINVAL, "row-slab mode needs nx >= 2 (got %d)", nx);
    if (NY / n < SLAB_HALO) return fail(DEFF_EINVAL, "%d rows over %d %s: fewer than %d rows per slab", NY, n, parts, SLAB_HALO);
    return DEFF_OK;
}

// Slab r of n of an nx x NY image on `device`: its context, copy stream and events.  On failure, slab_close releases what
// was made.
static int slab_open(Slab *s, int device, int nx, int NY, int n, int r)
{
    s->g0 = slab_first(NY, n, r);
    s->own = slab_first(NY, n, r + 1) - s->g0;
    TRY(deff_create_batch(device, nx, s->own + 2 * SLAB_HALO, 1, &s->c));
    deff_ctx *c = s->c;
    c->slab = true;
    c->halo = SLAB_HALO;
    c->dom_lo = SLAB_HALO - s->g0;            // array row of mesh row 0
    c->mesh_ny = NY;
    c->own_lo = SLAB_HALO;
    c->own_h = s->own;
    c->dy = 1.0 / NY;                         // the mesh is the whole image, cuh:1911
    c->kernel = DEFF_KERNEL_MATFREE_TB;
    // one T per IMAGE: keyed on the largest slab's array, a function of (nx, NY, n) only
    c->tb_ref_cells = (size_t)c->nx * (size_t)((NY + n - 1) / n + 2 * SLAB_HALO);
    hipError_t he;
    if ((he = hipSetDevice(device)) != hipSuccess ||
        (he = hipStreamCreateWithFlags(&s->xs, hipStreamNonBlocking)) != hipSuccess ||
        (he = hipEventCreateWithFlags(&s->bnd, hipEventDisableTiming)) != hipSuccess ||
        (he = hipEventCreateWithFlags(&s->halo, hipEventDisableTiming)) != hipSuccess)
        return fail(DEFF_EHIP, "stream / event creation failed: %s", hipGetErrorString(he));
    return DEFF_OK;
}

static void slab_close(Slab &s)
{
    if (!s.c) return;
    (void)hipSetDevice(s.c->device);
    if (s.xs) { (void)hipStreamSynchronize(s.xs); (void)hipStreamDestroy(s.xs); }
    if (s.bnd) (void)hipEventDestroy(s.bnd);
    if (s.halo) (void)hipEventDestroy(s.halo);
    if (s.cg_ev) (void)hipEventDestroy(s.cg_ev);
    if (s.cg_all) (void)hipFree(s.cg_all);
    deff_destroy(s.c);
    s.c = nullptr;
}

// The mesh rows a slab's arrays hold (own rows + halo, clipped to the mesh): the first one, its array row, their count.
struct SlabWindow {
    int first, array_first, count;
};
static SlabWindow slab_window(const Slab &s)
{
    const deff_ctx *c = s.c;
    int a = -c->dom_lo, b = a + c->rows;        // mesh rows covered by the array
    int ar = 0;
    if (a < 0) { ar = -a; a = 0; }
    if (b > c->mesh_ny) b = c->mesh_ny;
    return SlabWindow{a, ar, b - a};
}

// pix_window: the window's rows of the image (mesh amplification is not supported in slab mode)
static int slab_set_pixels(Slab &s, const uint8_t *pix_window)
{
    deff_ctx *c = s.c;
    TRY(use_device(c));
    TRY(image_shape(c, c->nxt, c->ny, 1, 1));
    HIP_TRY(hipMemsetAsync(c->pix, 0, (size_t)c->nxt * c->rows, c->stream));
    const SlabWindow w = slab_window(s);
    HIP_TRY(hipMemcpyAsync(c->pix + (size_t)w.array_first * c->nxt, pix_window, (size_t)w.count * c->nxt,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_image = true; c->have_matfree = false;
    return DEFF_OK;
}

static int slab_synth_image(Slab &s, uint64_t seed, uint64_t img)
{
    deff_ctx *c = s.c;
    TRY(use_device(c));
    TRY(image_shape(c, c->nxt, c->ny, 1, 1));
    HIP_TRY(hipMemsetAsync(c->pix, 0, (size_t)c->nxt * c->rows, c->stream));
    const SlabWindow w = slab_window(s);
    // the generator's key is seed*K + img*NY*nx + global cell index: start it at the window's first mesh row
    const uint64_t base_img_cells = img * (uint64_t)c->mesh_ny * (uint64_t)c->nxt + (uint64_t)w.first * (uint64_t)c->nxt;
    hipLaunchKernelGGL(k_synth_mask_at, dim3(grid_for((size_t)w.count * c->nxt)), dim3(256), 0, c->stream,
                       c->pix + (size_t)w.array_first * c->nxt, (size_t)w.count * c->nxt, seed, base_img_cells);
    HIP_TRY(hipGetLastError());
    c->have_image = true; c->have_matfree = false;
    return DEFF_OK;
}

// 3-phase system of one slab (deff_assemble_3phase): Grid_window is the window's rows of the image's flood-fill result
// (or NULL).  The explicit planes are harvested into a row dictionary per slab at the first sweep, so the slabs still run
// on the temporally blocked kernel; a system with too many distinct rows is refused by the sweep planner.
static int slab_assemble_3phase(Slab &s, double Ds, double Df, double Dg, const unsigned int *Grid_window, double CL,
                                double CR)
{
    deff_ctx *c = s.c;
    std::vector<unsigned int> win;
    if (Grid_window) {
        const SlabWindow w = slab_window(s);
        win.assign((size_t)c->rows * c->nxt, 0u);
        memcpy(&win[(size_t)w.array_first * c->nxt], Grid_window, sizeof(unsigned int) * (size_t)w.count * c->nxt);
    }
    return deff_assemble_3phase(c, Ds, Df, Dg, Grid_window ? win.data() : nullptr, CL, CR);
}

// own rows of the current field -> host, enqueued on the slab's stream
static int slab_get_own(Slab &s, double *x_own)
{
    deff_ctx *c = s.c;
    TRY(use_device(c));
    return rows_d2h(c, x_own, (const double *)(c->x[c->cur] + (size_t)c->own_lo * c->nx), (size_t)c->own_h);
}

// The T and T = 1 pass plans of every slab of the set.
static int slab_plans(const SlabSet &set, double omega)
{
    for (int r = 0; r < set.n; ++r) {
        Slab &s = set.s[r];
        deff_ctx *c = s.c;
        TRY(use_device(c));
        if (c->tb_T > SLAB_HALO) return fail(DEFF_EINVAL, "tb_T exceeds the slab halo depth %d", SLAB_HALO);
        TRY(slab_pass_plans(c, omega, 0, set.overlap, &s.plT));
        TRY(slab_pass_plans(c, omega, 1, set.overlap, &s.pl1));
        c->last_launches = 0;
        // all slabs of one image advance in lock-step: one T, one exchange per pass
        if (s.plT.whole.T != set.s[0].plT.whole.T)
            return fail(DEFF_ESTATE, "slab %d plans %d sweeps per pass, slab 0 plans %d: set tb_T on the group, not per slab", r,
                        s.plT.whole.T, set.s[0].plT.whole.T);
    }
    return DEFF_OK;
}

// n sweeps on every slab of the set: blocked passes of T, the remainder as T = 1 passes, one exchange per pass.
// Per pass, first per slab on its own stream: wait until its halo rows are valid (`halo`, recorded by the previous pass's
// exchange), sweep the two bands its neighbours wait for, record `bnd`, sweep the interior.  Then per slab on its copy
// stream xs (the context's stream when overlap is off): the exchange, which waits for the `bnd` of the rows it moves and
// brings the neighbours' new boundary rows into this slab's halo rows of the NEW field, then `halo`.  So the exchange of
// pass p runs while the interiors of pass p are still being swept, and pass p+1 of a slab starts as soon as ITS halos are
// in -- no global synchronisation.  Buffer reuse is safe by transitivity: a slab overwrites the rows a neighbour copied
// from two passes later, and it cannot get there before that neighbour recorded the `bnd` of the pass in between, which
// it does only after its copies finished.  A slab that is the whole image has no neighbour: no exchange, no `halo`.
static int slab_sweeps(const SlabSet &set, int64_t n)
{
    const int T = set.s[0].plT.whole.T;
    while (n > 0) {
        const bool big = n >= T;
        for (int r = 0; r < set.n; ++r) {
            Slab &s = set.s[r];
            TRY(use_device(s.c));
            HIP_TRY(hipStreamWaitEvent(s.c->stream, s.halo, 0));         // never recorded yet: returns at once
            TRY(slab_enqueue_pass(s.c, big ? s.plT : s.pl1, s.bnd));
        }
        for (int r = 0; r < set.n; ++r) {
            Slab &s = set.s[r];
            if (s.own == s.c->mesh_ny) continue;
            TRY(use_device(s.c));
            hipStream_t xs = set.overlap ? s.xs : s.c->stream;
            TRY(set.exchange(r, xs));
            HIP_TRY(hipEventRecord(s.halo, xs));
        }
        n -= big ? T : 1;
    }
    // whatever comes next on a slab's stream (fluxes, field download, another solve) sees complete halos
    for (int r = 0; r < set.n; ++r) {
        TRY(use_device(set.s[r].c));
        HIP_TRY(hipStreamWaitEvent(set.s[r].c->stream, set.s[r].halo, 0));
    }
    return DEFF_OK;
}

// Ends the window that ev0 of slab 0's context opened: the other slabs' streams are waited for on the host, slab 0's by
// ev1 itself.  *ms (may be NULL): the device time.
static int slab_elapsed(const SlabSet &set, float *ms)
{
    for (int r = 1; r < set.n; ++r) { TRY(use_device(set.s[r].c)); HIP_TRY(hipStreamSynchronize(set.s[r].c->stream)); }
    deff_ctx *c0 = set.s[0].c;
    TRY(use_device(c0));
    HIP_TRY(hipEventRecord(c0->ev1, c0->stream));
    HIP_TRY(hipEventSynchronize(c0->ev1));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, c0->ev0, c0->ev1));
    return DEFF_OK;
}

static int slab_timed_sweeps(const SlabSet &set, int64_t n, double omega, float *ms)
{
    TRY(slab_plans(set, omega));
    deff_ctx *c0 = set.s[0].c;
    TRY(use_device(c0));
    HIP_TRY(hipEventRecord(c0->ev0, c0->stream));
    TRY(slab_sweeps(set, n));
    return slab_elapsed(set, ms);
}

// JacobiGPU's loop (cuh:1232-1290) over the slabs, with the stopping rule of deff_solve.  flux(&deff) sums the wall
// fluxes of the whole image in global row order, so every slab / rank takes the same stop/continue decision.
static int slab_solve(const SlabSet &set, const std::function<int(double *deff_raw)> &flux, double omega, double tol,
                      int64_t max_iter, int64_t check_every, deff_result *out)
{
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    TRY(slab_plans(set, omega));
    deff_ctx *c0 = set.s[0].c;
    TRY(use_device(c0));
    HIP_TRY(hipEventRecord(c0->ev0, c0->stream));
    JacobiCheck chk;
    int64_t iter = 0;
    while (iter < max_iter && chk.more(tol)) {                       // cuh:1232
        const CheckStep st = check_step(iter, max_iter, check_every);
        TRY(slab_sweeps(set, st.sweeps));
        iter += st.sweeps;
        if (st.check) {
            double deff = 0;
            TRY(flux(&deff));
            chk.update(deff);
        }
    }
    float ms = 0;
    TRY(slab_elapsed(set, &ms));
    *out = chk.result(iter, ms);
    return DEFF_OK;
}

// ------------------------------------------------------------ conjugate gradients over the slabs --
//
// deff_solve_cg's loop (api_cg.hip) with the image's rows on several slabs: kernels_cg_slab.hpp has the dependency argument.
// Per iteration and slab: dir + slab sum | gather A | alpha, update + slab sums | one row of r to each neighbour, gather B |
// beta.  Every slab holds the same scalars bit for bit and freezes itself on the device; the host enqueues check_every
// iterations on every slab without waiting and then reads slab 0's state (set.s[0]: in the rank form, this rank's own).
// Between slabs only events order the work (cg_ev: "my rows and my slot are written"), recorded for all slabs before any
// slab waits for one.  The three gather phases have buffers of their own, so a slab's next sum never overwrites a slot a
// copy still reads: the gather in between is a barrier among all slabs ("Row slabs").

static double *slab_cg_r(const Slab &s) { return s.c->cg_r; }

// the 8-row exchange of the current field, as after a pass: every halo row of every slab holds the neighbours' rows
static int slab_exchange_field(const SlabSet &set)
{
    for (int r = 0; r < set.n; ++r) {
        TRY(use_device(set.s[r].c));
        HIP_TRY(hipEventRecord(set.s[r].bnd, set.s[r].c->stream));
    }
    for (int r = 0; r < set.n; ++r) {
        Slab &s = set.s[r];
        TRY(use_device(s.c));
        TRY(set.exchange(r, s.c->stream));
        HIP_TRY(hipEventRecord(s.halo, s.c->stream));
    }
    for (int r = 0; r < set.n; ++r) { TRY(use_device(set.s[r].c)); TRY(set.settle(r)); }
    return DEFF_OK;
}

static int slab_cg_record(const SlabSet &set, int r)
{
    HIP_TRY(hipEventRecord(set.s[r].cg_ev, set.s[r].c->stream));
    return DEFF_OK;
}

static int slab_solve_cg(const SlabSet &set, const std::function<int(double *deff_raw)> &flux, double rtol, int64_t max_iter,
                         int64_t check_every, deff_cg_result *out)
{
    const bool multi = set.total > 1;
    const size_t all_n = (size_t)CG_SLAB_PHASES * set.total * CG_SLAB_SLOT;
    for (int r = 0; r < set.n; ++r) {
        Slab &s = set.s[r];
        TRY(use_device(s.c));
        // x[cur] as it stands is the guess: a slab context is one image (nothing to consolidate) and never sweeps with
        // resident launches (resident_allowed), so this settles nothing today and stays right if that changes
        TRY(resident_check(s.c));
        if (!s.cg_all) {
            HIP_TRY(hipMalloc((void **)&s.cg_all, sizeof(double) * all_n));
            HIP_TRY(hipMemsetAsync(s.cg_all, 0, sizeof(double) * all_n, s.c->stream));
            HIP_TRY(hipEventCreateWithFlags(&s.cg_ev, hipEventDisableTiming));
        }
        s.cg.c = s.c;
        s.cg.nslabs = set.total;
        s.cg.me = set.first + r;
        s.cg.all = s.cg_all;
        TRY(slcg_setup(&s.cg, rtol, max_iter));
        TRY(slab_cg_record(set, r));
    }
    // the verdicts, gathered like a sum: every slab (every rank) sees them all and refuses or goes on with the others
    std::vector<double> verdict((size_t)set.total * CG_SLAB_SLOT);
    for (int r = 0; r < set.n; ++r) {
        Slab &s = set.s[r];
        TRY(use_device(s.c));
        if (multi) TRY(set.gather(r, 2));
        HIP_TRY(hipMemcpyAsync(verdict.data(), slcg_slot(s.cg, 2, 0), sizeof(double) * verdict.size(), hipMemcpyDeviceToHost,
                               s.c->stream));
        HIP_TRY(hipStreamSynchronize(s.c->stream));
    }
    for (int q = 0; q < set.total; ++q) {
        const double v = verdict[(size_t)q * CG_SLAB_SLOT];
        if (v == 0.0) continue;
        if (v == 1.0)
            return fail(DEFF_EINVAL, "CG over row slabs: the system is not symmetric (slab %d: a link between two active cells "
                                     "differs from its partner, or an active row links out of the image)", q);
        // the status of that slab's own checks, as deff_solve_cg gives it (slcg_setup: v = 1 - status)
        const int code = 1 - (int)v, r = q - set.first;
        const int status = code == DEFF_ESTATE || code == DEFF_ENOMEM ? code : DEFF_EINVAL;
        if (r >= 0 && r < set.n && !set.s[r].cg.refusal.empty())
            return fail(status, "CG over row slabs, slab %d: %s", q, std::string(set.s[r].cg.refusal).c_str());
        return fail(status, "CG over row slabs: slab %d cannot run it (its rank reports why)", q);
    }
    for (int r = 0; r < set.n; ++r) slcg_commit(&set.s[r].cg);

    deff_ctx *c0 = set.s[0].c;
    TRY(use_device(c0));
    HIP_TRY(hipEventRecord(c0->ev0, c0->stream));
    // r = b - A x and its check on every slab: x's halo rows first, r's adjacent halo row afterwards
    auto residual_round = [&](int mode, int allow) -> int {
        if (multi) TRY(slab_exchange_field(set));
        for (int r = 0; r < set.n; ++r) {
            TRY(use_device(set.s[r].c));
            TRY(slcg_resid(&set.s[r].cg));
            TRY(slab_cg_record(set, r));
        }
        for (int r = 0; r < set.n; ++r) {
            TRY(use_device(set.s[r].c));
            if (multi) { TRY(set.send_row(r, slab_cg_r)); TRY(set.gather(r, 2)); }
            TRY(slcg_check(&set.s[r].cg, mode, allow));
        }
        return DEFF_OK;
    };
    // the one host wait of an interval: slab 0's scalars (every slab's are the same bits), every slab's stream idle
    CgSlabState st;
    auto look = [&]() -> int {
        TRY(use_device(c0));
        TRY(slcg_read(&set.s[0].cg, &st));
        for (int r = 1; r < set.n; ++r) { TRY(use_device(set.s[r].c)); HIP_TRY(hipStreamSynchronize(set.s[r].c->stream)); }
        return DEFF_OK;
    };
    TRY(residual_round(0, 0));
    int rounds = 0;
    for (;;) {
        TRY(look());
        if (st.done) {
            // the recurrence's residual drifts from b - A x: recompute it; a solve whose true residual misses rtol goes on
            TRY(residual_round(1, rounds < CG_MAX_RESTARTS));
            TRY(look());
            if (!st.restarted) break;
            ++rounds;
            for (int r = 0; r < set.n; ++r) set.s[r].c->cg_plan_restarts = rounds;
        }
        for (int64_t i = 0; i < check_every; ++i) {
            for (int r = 0; r < set.n; ++r) {
                TRY(use_device(set.s[r].c));
                TRY(slcg_dir(&set.s[r].cg));
                if (multi) TRY(slab_cg_record(set, r));
            }
            // every slab's wait on the others' dir is enqueued before any slab records its update: a wait binds to the
            // event's latest record, and behind a neighbour's newer one the updates would run one slab after another
            if (multi)
                for (int r = 0; r < set.n; ++r) { TRY(use_device(set.s[r].c)); TRY(set.gather(r, 0)); }
            for (int r = 0; r < set.n; ++r) {
                TRY(use_device(set.s[r].c));
                TRY(slcg_alpha_update(&set.s[r].cg));
                if (multi) TRY(slab_cg_record(set, r));
            }
            for (int r = 0; r < set.n; ++r) {
                TRY(use_device(set.s[r].c));
                if (multi) { TRY(set.send_row(r, slab_cg_r)); TRY(set.gather(r, 1)); }
                TRY(slcg_beta(&set.s[r].cg));
            }
        }
    }
    // an ordinary slab set again: the last round wrote zeros on decoupled cells, so the field's halo rows travel once more
    if (multi) TRY(slab_exchange_field(set));
    float ms = 0;
    TRY(slab_elapsed(set, &ms));
    double deff = 0;
    TRY(flux(&deff));
    out->iters = st.iters;
    out->rel_residual = st.rel;
    out->deff_raw = deff;
    out->loop_ms = ms;
    out->converged = st.rel <= rtol;
    return DEFF_OK;
}

static int cg_arguments(const void *obj, const deff_cg_result *out, double rtol, int64_t max_iter, int64_t check_every)
{
    if (!obj || !out) return fail(DEFF_EINVAL, "NULL argument");
    if (!(rtol >= 0.0) || !std::isfinite(rtol)) return fail(DEFF_EINVAL, "CG over row slabs: rtol must be finite and >= 0");
    if (max_iter < 0) return fail(DEFF_EINVAL, "CG over row slabs: negative max_iter");
    if (check_every < 1) return fail(DEFF_EINVAL, "check_every must be >= 1");
    return DEFF_OK;
}

// --------------------------------------------------------- row slabs, one process, N devices --

struct deff_slab_group {
    std::vector<Slab> slabs;
    int NY = 0;
    int overlap = 1;
    std::vector<double> mfl, mfr;             // global wall fluxes of the last check
};

extern "C" int deff_slab_group_destroy(deff_slab_group *g)
try {
    if (!g) return DEFF_OK;
    for (Slab &s : g->slabs) slab_close(s);
    delete g;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_create(int nslabs, const int *devices, int nx, int NY, deff_slab_group **out)
try {
    if (!out || nslabs < 1) return fail(DEFF_EINVAL, "bad slab group arguments");
    *out = nullptr;
    TRY(slab_check(nx, NY, nslabs, "slabs"));
    deff_slab_group *g = new (std::nothrow) deff_slab_group();
    if (!g) return fail(DEFF_ENOMEM, "host allocation failed");
    g->NY = NY;
    g->mfl.assign(NY, 0.0); g->mfr.assign(NY, 0.0);
    g->slabs.resize(nslabs);
    int rc = DEFF_OK;
    for (int r = 0; r < nslabs && rc == DEFF_OK; ++r) rc = slab_open(&g->slabs[r], devices ? devices[r] : 0, nx, NY, nslabs, r);
    if (rc != DEFF_OK) { deff_slab_group_destroy(g); return rc; }
    // direct xGMI copies between neighbouring slabs' devices (staged through the host otherwise)
    for (int r = 0; r + 1 < nslabs; ++r) {
        const int a = g->slabs[r].c->device, b = g->slabs[r + 1].c->device;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) {
            (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0);
            (void)hipSetDevice(b); (void)hipDeviceEnablePeerAccess(a, 0);
            (void)hipGetLastError();                 // "already enabled" is fine
        }
    }
    *out = g;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_layout(const deff_slab_group *g, int *first_row, int *row_count)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    for (size_t r = 0; r < g->slabs.size(); ++r) {
        if (first_row) first_row[r] = g->slabs[r].g0;
        if (row_count) row_count[r] = g->slabs[r].own;
    }
    return DEFF_OK;
}
DEFF_API_CATCH

// pix: the whole image, NY x nx bytes
extern "C" int deff_slab_group_set_image(deff_slab_group *g, const uint8_t *pix)
try {
    if (!g || !pix) return fail(DEFF_EINVAL, "NULL argument");
    for (Slab &s : g->slabs) TRY(slab_set_pixels(s, pix + (size_t)slab_window(s).first * s.c->nxt));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_synth_image(deff_slab_group *g, uint64_t seed, uint64_t img)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    for (Slab &s : g->slabs) TRY(slab_synth_image(s, seed, img));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_assemble_2phase(deff_slab_group *g, double Ds, double Df, double CL, double CR)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    for (Slab &s : g->slabs) TRY(deff_assemble_2phase(s.c, Ds, Df, CL, CR));
    return DEFF_OK;
}
DEFF_API_CATCH

// Grid: the whole image's flood-fill result (NY x nx, may be NULL)
extern "C" int deff_slab_group_assemble_3phase(deff_slab_group *g, double Ds, double Df, double Dg,
                                               const unsigned int *Grid, double CL, double CR)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    for (Slab &s : g->slabs)
        TRY(slab_assemble_3phase(s, Ds, Df, Dg, Grid ? Grid + (size_t)slab_window(s).first * s.c->nxt : nullptr, CL, CR));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_init_linear(deff_slab_group *g, double CL, double CR)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    for (Slab &s : g->slabs) TRY(deff_init_linear(s.c, CL, CR));     // a function of the column only
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_set_field(deff_slab_group *g, const double *x)
try {
    if (!g || !x) return fail(DEFF_EINVAL, "NULL argument");
    for (Slab &s : g->slabs) {
        deff_ctx *c = s.c;
        TRY(use_device(c));
        HIP_TRY(hipMemsetAsync(c->x[c->cur], 0, sizeof(double) * c->n, c->stream));
        const SlabWindow w = slab_window(s);
        TRY(rows_h2d(c, c->x[c->cur] + (size_t)w.array_first * c->nx, x + (size_t)w.first * c->nxt, (size_t)w.count));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->have_field = true;
        reset_batch_state(c);
    }
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_get_field(deff_slab_group *g, double *x)
try {
    if (!g || !x) return fail(DEFF_EINVAL, "NULL argument");
    for (Slab &s : g->slabs) TRY(slab_get_own(s, x + (size_t)s.g0 * s.c->nxt));
    for (Slab &s : g->slabs) { TRY(use_device(s.c)); HIP_TRY(hipStreamSynchronize(s.c->stream)); }
    return DEFF_OK;
}
DEFF_API_CATCH

// The group's exchange for slab r: its neighbours' new boundary rows are copied into its halo rows (hipMemcpyPeerAsync:
// xGMI between devices), each copy behind that neighbour's `bnd`.
static int group_exchange(deff_slab_group *g, int r, hipStream_t xs)
{
    deff_ctx *c = g->slabs[r].c;
    const size_t bytes = sizeof(double) * SLAB_HALO * c->nx;
    if (r > 0) {                                                   // top halo <- last own rows of slab r-1
        const Slab &u = g->slabs[r - 1];
        HIP_TRY(hipStreamWaitEvent(xs, u.bnd, 0));
        const double *src = u.c->x[u.c->cur] + (size_t)(u.c->own_lo + u.c->own_h - SLAB_HALO) * c->nx;
        HIP_TRY(hipMemcpyPeerAsync(c->x[c->cur], c->device, src, u.c->device, bytes, xs));
    }
    if (r + 1 < (int)g->slabs.size()) {                            // bottom halo <- first own rows of slab r+1
        const Slab &d = g->slabs[r + 1];
        HIP_TRY(hipStreamWaitEvent(xs, d.bnd, 0));
        const double *src = d.c->x[d.c->cur] + (size_t)d.c->own_lo * c->nx;
        HIP_TRY(hipMemcpyPeerAsync(c->x[c->cur] + (size_t)(c->own_lo + c->own_h) * c->nx, c->device, src, d.c->device,
                                   bytes, xs));
    }
    return DEFF_OK;
}

static SlabSet slabs_of(deff_slab_group *g)
{
    return SlabSet{g->slabs.data(), (int)g->slabs.size(), g->overlap,
                   [g](int r, hipStream_t xs) { return group_exchange(g, r, xs); }};
}

extern "C" int deff_slab_group_sweeps(deff_slab_group *g, int64_t n, double omega, float *ms)
try {
    if (!g || n < 0) return fail(DEFF_EINVAL, "bad arguments");
    return slab_timed_sweeps(slabs_of(g), n, omega, ms);
}
DEFF_API_CATCH

// Wall fluxes of every slab's own rows -> the group's global arrays -> Deff (cuh:1252-1263).
static int group_flux(deff_slab_group *g, double *deff_raw)
{
    for (Slab &s : g->slabs) { TRY(use_device(s.c)); TRY(flux_rows(s.c)); }
    for (const Slab &s : g->slabs) {
        memcpy(&g->mfl[s.g0], s.c->mf_host + s.c->own_lo, sizeof(double) * s.own);
        memcpy(&g->mfr[s.g0], s.c->mf_host + s.c->rows + s.c->own_lo, sizeof(double) * s.own);
    }
    const deff_ctx *c = g->slabs[0].c;
    *deff_raw = deff_of_fluxes(g->mfl.data(), g->mfr.data(), g->NY, c->CL, c->CR);
    return DEFF_OK;
}

extern "C" int deff_slab_group_flux(deff_slab_group *g, double *deff_raw, double *MFL, double *MFR)
try {
    if (!g || !deff_raw) return fail(DEFF_EINVAL, "NULL argument");
    TRY(group_flux(g, deff_raw));
    if (MFL) memcpy(MFL, g->mfl.data(), sizeof(double) * g->NY);
    if (MFR) memcpy(MFR, g->mfr.data(), sizeof(double) * g->NY);
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_solve(deff_slab_group *g, double omega, double tol, int64_t max_iter,
                                     int64_t check_every, deff_result *out, double *MFL, double *MFR)
try {
    if (!g || !out) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_solve(slabs_of(g), [g](double *deff_raw) { return group_flux(g, deff_raw); }, omega, tol, max_iter,
                   check_every, out));
    if (MFL) memcpy(MFL, g->mfl.data(), sizeof(double) * g->NY);
    if (MFR) memcpy(MFR, g->mfr.data(), sizeof(double) * g->NY);
    return DEFF_OK;
}
DEFF_API_CATCH

// The group's transports for conjugate gradients, all on slab r's own stream behind the other slabs' cg_ev.
static int group_send_row(deff_slab_group *g, int r, double *(*buf)(const Slab &))
{
    const Slab &me = g->slabs[r];
    deff_ctx *c = me.c;
    const size_t bytes = sizeof(double) * c->nx;
    if (r > 0) {                                                   // halo row above <- last own row of slab r-1
        const Slab &u = g->slabs[r - 1];
        HIP_TRY(hipStreamWaitEvent(c->stream, u.cg_ev, 0));
        HIP_TRY(hipMemcpyPeerAsync(buf(me) + (size_t)(c->own_lo - 1) * c->nx, c->device,
                                   buf(u) + (size_t)(u.c->own_lo + u.c->own_h - 1) * c->nx, u.c->device, bytes, c->stream));
    }
    if (r + 1 < (int)g->slabs.size()) {                            // halo row below <- first own row of slab r+1
        const Slab &d = g->slabs[r + 1];
        HIP_TRY(hipStreamWaitEvent(c->stream, d.cg_ev, 0));
        HIP_TRY(hipMemcpyPeerAsync(buf(me) + (size_t)(c->own_lo + c->own_h) * c->nx, c->device,
                                   buf(d) + (size_t)d.c->own_lo * c->nx, d.c->device, bytes, c->stream));
    }
    return DEFF_OK;
}

static int group_gather(deff_slab_group *g, int r, int phase)
{
    const Slab &me = g->slabs[r];
    for (int q = 0; q < (int)g->slabs.size(); ++q) {
        if (q == r) continue;
        const Slab &o = g->slabs[q];
        HIP_TRY(hipStreamWaitEvent(me.c->stream, o.cg_ev, 0));
        HIP_TRY(hipMemcpyPeerAsync(slcg_slot(me.cg, phase, q), me.c->device, slcg_slot(o.cg, phase, q), o.c->device,
                                   sizeof(double) * CG_SLAB_SLOT, me.c->stream));
    }
    return DEFF_OK;
}

// slab r goes on only when its neighbours' copies out of its rows are done (their `halo`)
static int group_settle(deff_slab_group *g, int r)
{
    if (r > 0) HIP_TRY(hipStreamWaitEvent(g->slabs[r].c->stream, g->slabs[r - 1].halo, 0));
    if (r + 1 < (int)g->slabs.size()) HIP_TRY(hipStreamWaitEvent(g->slabs[r].c->stream, g->slabs[r + 1].halo, 0));
    return DEFF_OK;
}

static SlabSet cg_slabs_of(deff_slab_group *g)
{
    SlabSet set = slabs_of(g);
    set.total = (int)g->slabs.size();
    set.first = 0;
    set.send_row = [g](int r, double *(*buf)(const Slab &)) { return group_send_row(g, r, buf); };
    set.gather = [g](int r, int phase) { return group_gather(g, r, phase); };
    set.settle = [g](int r) { return group_settle(g, r); };
    return set;
}

extern "C" int deff_slab_group_solve_cg(deff_slab_group *g, double rtol, int64_t max_iter, int64_t check_every,
                                        deff_cg_result *out, double *MFL, double *MFR)
try {
    TRY(cg_arguments(g, out, rtol, max_iter, check_every));
    TRY(slab_solve_cg(cg_slabs_of(g), [g](double *deff_raw) { return group_flux(g, deff_raw); }, rtol, max_iter, check_every,
                      out));
    if (MFL) memcpy(MFL, g->mfl.data(), sizeof(double) * g->NY);
    if (MFR) memcpy(MFR, g->mfr.data(), sizeof(double) * g->NY);
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_set_tuning(deff_slab_group *g, const char *key, int value)
try {
    if (!g) return fail(DEFF_EINVAL, "group is NULL");
    if (key && !strcmp(key, "slab_overlap")) { g->overlap = value > 2 ? 2 : value; return DEFF_OK; }
    for (Slab &s : g->slabs) TRY(deff_set_tuning(s.c, key, value));
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_group_get_plan(deff_slab_group *g, int slab, const char *key, int *value)
try {
    if (!g || slab < 0 || slab >= (int)g->slabs.size()) return fail(DEFF_EINVAL, "bad slab index");
    return deff_get_plan(g->slabs[slab].c, key, value);
}
DEFF_API_CATCH

// ------------------------------------------------- row slabs, one process per GPU (RCCL) --
//
// Same slab and the same loops as the group above; only the transport differs: the halo
// blocks travel by grouped ncclSend/ncclRecv between neighbouring ranks on the context's stream
// (point-to-point over one xGMI link per neighbour pair; 8 rows x nx doubles, 1 MiB at nx =
// 16384, once per blocked pass), and the per-row wall fluxes are all-gathered so that every rank
// sums them in global row order and takes the same stop/continue decision.

struct deff_slab_rank {
    Slab slab;
    int rank = 0, nranks = 1, NY = 0, maxown = 0;    // maxown: rows of the largest slab
    ncclComm_t comm = nullptr;
    double *d_pack = nullptr, *d_all = nullptr;      // [2*maxown], [nranks*2*maxown]
    std::vector<double> h_all, mfl, mfr;
    // host-staged custom transport (deff_slab_rank_create_custom): the same loop, the blocks go
    // through host buffers and the caller's callbacks instead of RCCL
    deff_host_exchange_fn xchg = nullptr;
    deff_host_allgather_fn gather = nullptr;
    void *user = nullptr;
    std::vector<double> h_send_up, h_send_dn, h_recv_up, h_recv_dn, h_pack;
    std::vector<double> h_cg_all;                    // ... and the gathered sums of conjugate gradients
    int overlap = 1;
};

#define NCCL_TRY(expr)                                                                          \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail(DEFF_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

extern "C" int deff_rccl_unique_id(char *id128)
try {
    if (!id128) return fail(DEFF_EINVAL, "id buffer is NULL");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_rank_destroy(deff_slab_rank *s)
try {
    if (!s) return DEFF_OK;
    slab_close(s->slab);                             // first: waits for the slab's streams
    if (s->d_pack) (void)hipFree(s->d_pack);
    if (s->d_all) (void)hipFree(s->d_all);
    if (s->comm) (void)ncclCommDestroy(s->comm);
    delete s;
    return DEFF_OK;
}
DEFF_API_CATCH

static int slab_rank_create_impl(int device, int nx, int NY, int rank, int nranks, const char *id128,
                                 deff_host_exchange_fn xchg, deff_host_allgather_fn gather, void *user,
                                 deff_slab_rank **out)
{
    if (!out || nranks < 1 || rank < 0 || rank >= nranks) return fail(DEFF_EINVAL, "bad slab rank arguments");
    *out = nullptr;
    TRY(slab_check(nx, NY, nranks, "ranks"));
    deff_slab_rank *s = new (std::nothrow) deff_slab_rank();
    if (!s) return fail(DEFF_ENOMEM, "host allocation failed");
    s->rank = rank; s->nranks = nranks; s->NY = NY;
    for (int r = 0; r < nranks; ++r) s->maxown = std::max(s->maxown, slab_first(NY, nranks, r + 1) - slab_first(NY, nranks, r));
    s->mfl.assign(NY, 0.0); s->mfr.assign(NY, 0.0);
    s->h_all.assign((size_t)nranks * 2 * s->maxown, 0.0);
    s->xchg = xchg; s->gather = gather; s->user = user;
    // The grouped ncclSend/ncclRecv on a second stream, concurrent with the interior launch, has never run between two
    // ranks (no multi-GPU box in this pipeline): until it has, the RCCL transport exchanges on the solver's stream unless
    // the caller asks for the overlap (slab_overlap 1 / 2).  The host-staged transport is verified and keeps it.
    s->overlap = xchg ? 1 : 0;
    if (xchg) {
        const size_t blk = (size_t)SLAB_HALO * ((nx + 1) & ~1);   // the device rows' (even) width
        s->h_send_up.assign(blk, 0.0); s->h_send_dn.assign(blk, 0.0);
        s->h_recv_up.assign(blk, 0.0); s->h_recv_dn.assign(blk, 0.0);
        s->h_pack.assign((size_t)2 * s->maxown, 0.0);
    }
    int rc = slab_open(&s->slab, device, nx, NY, nranks, rank);
    if (rc == DEFF_OK) {
        ncclUniqueId id;
        if (id128) memcpy(&id, id128, sizeof id);
        hipError_t he;
        ncclResult_t nr;
        if ((he = hipSetDevice(device)) != hipSuccess) rc = fail(DEFF_EHIP, "hipSetDevice: %s", hipGetErrorString(he));
        else if (id128 && (nr = ncclCommInitRank(&s->comm, nranks, id, rank)) != ncclSuccess)
            rc = fail(DEFF_ECOMM, "ncclCommInitRank: %s", ncclGetErrorString(nr));
        else if ((he = hipMalloc((void **)&s->d_pack, sizeof(double) * 2 * s->maxown)) != hipSuccess ||
                 (he = hipMalloc((void **)&s->d_all, sizeof(double) * 2 * s->maxown * nranks)) != hipSuccess)
            rc = fail(DEFF_ENOMEM, "hipMalloc: %s", hipGetErrorString(he));
        else if ((he = hipMemset(s->d_pack, 0, sizeof(double) * 2 * s->maxown)) != hipSuccess)
            rc = fail(DEFF_EHIP, "hipMemset: %s", hipGetErrorString(he));
    }
    if (rc != DEFF_OK) { deff_slab_rank_destroy(s); return rc; }
    *out = s;
    return DEFF_OK;
}

extern "C" int deff_slab_rank_create(int device, int nx, int NY, int rank, int nranks, const char *id128,
                                     deff_slab_rank **out)
try {
    if (!id128) return fail(DEFF_EINVAL, "RCCL id is NULL");
    return slab_rank_create_impl(device, nx, NY, rank, nranks, id128, nullptr, nullptr, nullptr, out);
}
DEFF_API_CATCH

// Same slabs and loop with a caller-supplied transport: after every pass the two 8-row blocks are
// copied to the host and handed to `exchange`, the fluxes to `allgather` (both collective over the
// ranks).  Slow (host staged) but runs anywhere -- e.g. two processes sharing one GPU under gloo,
// which is how the per-rank loop is tested across real process boundaries.
extern "C" int deff_slab_rank_create_custom(int device, int nx, int NY, int rank, int nranks,
                                            deff_host_exchange_fn exchange, deff_host_allgather_fn allgather,
                                            void *user, deff_slab_rank **out)
try {
    if (!exchange || !allgather) return fail(DEFF_EINVAL, "transport callbacks are NULL");
    return slab_rank_create_impl(device, nx, NY, rank, nranks, nullptr, exchange, allgather, user, out);
}
DEFF_API_CATCH

extern "C" int deff_slab_rank_layout(const deff_slab_rank *s, int *first_row, int *row_count)
try {
    if (!s) return fail(DEFF_EINVAL, "slab is NULL");
    if (first_row) *first_row = s->slab.g0;
    if (row_count) *row_count = s->slab.own;
    return DEFF_OK;
}
DEFF_API_CATCH

// the context behind the slab, for deff_set_tuning / deff_assemble_2phase / deff_init_linear
extern "C" int deff_slab_rank_context(deff_slab_rank *s, deff_ctx **ctx)
try {
    if (!s || !ctx) return fail(DEFF_EINVAL, "NULL argument");
    *ctx = s->slab.c;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_rank_set_tuning(deff_slab_rank *s, const char *key, int value)
try {
    if (!s || !key) return fail(DEFF_EINVAL, "NULL argument");
    if (!strcmp(key, "slab_overlap")) { s->overlap = value > 2 ? 2 : value; return DEFF_OK; }
    return deff_set_tuning(s->slab.c, key, value);
}
DEFF_API_CATCH

// window = the rows of the whole image this rank's arrays cover (own rows + halo, clipped to the
// mesh): *first_row, *row_count; the image upload below takes exactly those rows.
extern "C" int deff_slab_rank_window(const deff_slab_rank *s, int *first_row, int *row_count)
try {
    if (!s) return fail(DEFF_EINVAL, "slab is NULL");
    const SlabWindow w = slab_window(s->slab);
    if (first_row) *first_row = w.first;
    if (row_count) *row_count = w.count;
    return DEFF_OK;
}
DEFF_API_CATCH

extern "C" int deff_slab_rank_set_image_window(deff_slab_rank *s, const uint8_t *pix_window)
try {
    if (!s || !pix_window) return fail(DEFF_EINVAL, "NULL argument");
    return slab_set_pixels(s->slab, pix_window);
}
DEFF_API_CATCH

// 3-phase system of this rank's slab; Grid_window = the rows deff_slab_rank_window() names of the
// image's flood-fill result (or NULL)
extern "C" int deff_slab_rank_assemble_3phase(deff_slab_rank *s, double Ds, double Df, double Dg,
                                              const unsigned int *Grid_window, double CL, double CR)
try {
    if (!s) return fail(DEFF_EINVAL, "slab is NULL");
    return slab_assemble_3phase(s->slab, Ds, Df, Dg, Grid_window, CL, CR);
}
DEFF_API_CATCH

extern "C" int deff_slab_rank_synth_image(deff_slab_rank *s, uint64_t seed, uint64_t img)
try {
    if (!s) return fail(DEFF_EINVAL, "slab is NULL");
    return slab_synth_image(s->slab, seed, img);
}
DEFF_API_CATCH

// own rows of the current field -> host
extern "C" int deff_slab_rank_get_field(deff_slab_rank *s, double *x_own)
try {
    if (!s || !x_own) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_get_own(s->slab, x_own));
    HIP_TRY(hipStreamSynchronize(s->slab.c->stream));
    return DEFF_OK;
}
DEFF_API_CATCH

// The rank's exchange after a pass, on stream `xs` (the copy stream when overlapping, else the context's), behind `bnd`:
// the first / last SLAB_HALO owned rows of the NEW field go to the neighbours, theirs come into the halo rows.
static int rank_exchange(deff_slab_rank *s, hipStream_t xs)
{
    deff_ctx *c = s->slab.c;
    const size_t blk = (size_t)SLAB_HALO * c->nx;
    double *x = c->x[c->cur];
    HIP_TRY(hipStreamWaitEvent(xs, s->slab.bnd, 0));
    if (s->xchg) {                                               // host-staged custom transport
        const bool up = s->rank > 0, dn = s->rank + 1 < s->nranks;
        double *top_own = x + (size_t)c->own_lo * c->nx, *bot_own = x + (size_t)(c->own_lo + c->own_h - SLAB_HALO) * c->nx;
        if (up) HIP_TRY(hipMemcpyAsync(s->h_send_up.data(), top_own, sizeof(double) * blk, hipMemcpyDeviceToHost, xs));
        if (dn) HIP_TRY(hipMemcpyAsync(s->h_send_dn.data(), bot_own, sizeof(double) * blk, hipMemcpyDeviceToHost, xs));
        HIP_TRY(hipStreamSynchronize(xs));                       // the interior of the pass keeps running on the other stream
        if (s->xchg(s->user, up ? s->h_send_up.data() : nullptr, up ? s->h_recv_up.data() : nullptr,
                    dn ? s->h_send_dn.data() : nullptr, dn ? s->h_recv_dn.data() : nullptr, blk) != 0)
            return fail(DEFF_ECOMM, "custom halo exchange failed");
        if (up) HIP_TRY(hipMemcpyAsync(x, s->h_recv_up.data(), sizeof(double) * blk, hipMemcpyHostToDevice, xs));
        if (dn) HIP_TRY(hipMemcpyAsync(x + (size_t)(c->own_lo + c->own_h) * c->nx, s->h_recv_dn.data(), sizeof(double) * blk,
                                       hipMemcpyHostToDevice, xs));
        HIP_TRY(hipStreamSynchronize(xs));                       // the host buffers are reused by the next pass
        return DEFF_OK;
    }
    // a failure between GroupStart and GroupEnd must still close the group, or every later collective
    // on this communicator is poisoned: remember the first error, always call ncclGroupEnd, then report
    NCCL_TRY(ncclGroupStart());
    ncclResult_t first = ncclSuccess;
    const char *what = "";
    auto step = [&](ncclResult_t r, const char *name) { if (first == ncclSuccess && r != ncclSuccess) { first = r; what = name; } };
    if (s->rank > 0) {
        step(ncclSend(x + (size_t)c->own_lo * c->nx, blk, ncclDouble, s->rank - 1, s->comm, xs), "ncclSend(up)");
        step(ncclRecv(x, blk, ncclDouble, s->rank - 1, s->comm, xs), "ncclRecv(up)");
    }
    if (s->rank + 1 < s->nranks) {
        step(ncclSend(x + (size_t)(c->own_lo + c->own_h - SLAB_HALO) * c->nx, blk, ncclDouble, s->rank + 1, s->comm, xs),
             "ncclSend(down)");
        step(ncclRecv(x + (size_t)(c->own_lo + c->own_h) * c->nx, blk, ncclDouble, s->rank + 1, s->comm, xs), "ncclRecv(down)");
    }
    const ncclResult_t end = ncclGroupEnd();
    if (first != ncclSuccess) return fail(DEFF_ECOMM, "%s failed: %s", what, ncclGetErrorString(first));
    if (end != ncclSuccess) return fail(DEFF_ECOMM, "ncclGroupEnd failed: %s", ncclGetErrorString(end));
    return DEFF_OK;
}

// a rank of one has no neighbour: its passes are never split (slab_overlap does not apply)
static SlabSet slabs_of(deff_slab_rank *s)
{
    return SlabSet{&s->slab, 1, s->nranks > 1 ? s->overlap : 0, [s](int, hipStream_t xs) { return rank_exchange(s, xs); }};
}

extern "C" int deff_slab_rank_sweeps(deff_slab_rank *s, int64_t n, double omega, float *ms)
try {
    if (!s || n < 0) return fail(DEFF_EINVAL, "bad arguments");
    return slab_timed_sweeps(slabs_of(s), n, omega, ms);
}
DEFF_API_CATCH

static __global__ void k_pack_own_flux(const double *__restrict__ mf, int rows, int own_lo, int own_h, int maxown,
                                double *__restrict__ pack)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= own_h) return;
    pack[i] = mf[own_lo + i];
    pack[maxown + i] = mf[rows + own_lo + i];
}

// Wall fluxes of this rank's own rows -> all-gathered into the global arrays -> Deff (cuh:1252-1263).
static int rank_flux(deff_slab_rank *s, double *deff_raw)
{
    deff_ctx *c = s->slab.c;
    if (!c->have_walls) return fail(DEFF_ESTATE, "wall diffusivities unknown");
    hipLaunchKernelGGL(k_wall_flux, dim3((c->rows + 255) / 256), dim3(256), 0, c->stream, c->x[c->cur], c->Dl, c->Dr,
                       c->nx, c->nxt, c->rows, c->dx, c->CL, c->CR, c->mf);
    hipLaunchKernelGGL(k_pack_own_flux, dim3((c->own_h + 255) / 256), dim3(256), 0, c->stream, c->mf, c->rows, c->own_lo,
                       c->own_h, s->maxown, s->d_pack);
    HIP_TRY(hipGetLastError());
    if (s->gather) {
        HIP_TRY(hipMemcpyAsync(s->h_pack.data(), s->d_pack, sizeof(double) * 2 * s->maxown, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (s->gather(s->user, s->h_pack.data(), s->h_all.data(), (size_t)2 * s->maxown) != 0)
            return fail(DEFF_ECOMM, "custom flux all-gather failed");
    } else {
        NCCL_TRY(ncclAllGather(s->d_pack, s->d_all, (size_t)2 * s->maxown, ncclDouble, s->comm, c->stream));
        HIP_TRY(hipMemcpyAsync(s->h_all.data(), s->d_all, sizeof(double) * s->h_all.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int r = 0; r < s->nranks; ++r) {
        const double *blk = s->h_all.data() + (size_t)r * 2 * s->maxown;
        const int g0 = slab_first(s->NY, s->nranks, r), own = slab_first(s->NY, s->nranks, r + 1) - g0;
        memcpy(&s->mfl[g0], blk, sizeof(double) * own);
        memcpy(&s->mfr[g0], blk + s->maxown, sizeof(double) * own);
    }
    *deff_raw = deff_of_fluxes(s->mfl.data(), s->mfr.data(), s->NY, c->CL, c->CR);
    return DEFF_OK;
}

// Collective over the ranks of the communicator: every rank calls it with the same arguments
// and gets the same result (iters, Deff, conv); MFL/MFR receive the GLOBAL fluxes (NY each).
extern "C" int deff_slab_rank_solve(deff_slab_rank *s, double omega, double tol, int64_t max_iter, int64_t check_every,
                                    deff_result *out, double *MFL, double *MFR)
try {
    if (!s || !out) return fail(DEFF_EINVAL, "NULL argument");
    TRY(slab_solve(slabs_of(s), [s](double *deff_raw) { return rank_flux(s, deff_raw); }, omega, tol, max_iter,
                   check_every, out));
    if (MFL) memcpy(MFL, s->mfl.data(), sizeof(double) * s->NY);
    if (MFR) memcpy(MFR, s->mfr.data(), sizeof(double) * s->NY);
    return DEFF_OK;
}
DEFF_API_CATCH

// The rank's transports for conjugate gradients, on the context's stream.  RCCL: a grouped ncclSend / ncclRecv of one row
// per neighbour and an in-place ncclAllGather of the slots, no host wait.  Custom: host staged through the caller's
// callbacks (`exchange` with count = row pitch, `allgather` with count = CG_SLAB_SLOT), which waits every time.
static int rank_send_row(deff_slab_rank *s, double *(*buf)(const Slab &))
{
    deff_ctx *c = s->slab.c;
    const size_t row = (size_t)c->nx;
    double *b = buf(s->slab);
    const bool up = s->rank > 0, dn = s->rank + 1 < s->nranks;
    double *top_own = b + (size_t)c->own_lo * row, *bot_own = b + (size_t)(c->own_lo + c->own_h - 1) * row;
    double *top_halo = b + (size_t)(c->own_lo - 1) * row, *bot_halo = b + (size_t)(c->own_lo + c->own_h) * row;
    if (s->xchg) {
        if (up) HIP_TRY(hipMemcpyAsync(s->h_send_up.data(), top_own, sizeof(double) * row, hipMemcpyDeviceToHost, c->stream));
        if (dn) HIP_TRY(hipMemcpyAsync(s->h_send_dn.data(), bot_own, sizeof(double) * row, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (s->xchg(s->user, up ? s->h_send_up.data() : nullptr, up ? s->h_recv_up.data() : nullptr,
                    dn ? s->h_send_dn.data() : nullptr, dn ? s->h_recv_dn.data() : nullptr, row) != 0)
            return fail(DEFF_ECOMM, "custom row exchange failed");
        if (up) HIP_TRY(hipMemcpyAsync(top_halo, s->h_recv_up.data(), sizeof(double) * row, hipMemcpyHostToDevice, c->stream));
        if (dn) HIP_TRY(hipMemcpyAsync(bot_halo, s->h_recv_dn.data(), sizeof(double) * row, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                // the host buffers are reused by the next exchange
        return DEFF_OK;
    }
    NCCL_TRY(ncclGroupStart());                                  // (a failure inside still closes the group: rank_exchange)
    ncclResult_t first = ncclSuccess;
    const char *what = "";
    auto step = [&](ncclResult_t r, const char *name) { if (first == ncclSuccess && r != ncclSuccess) { first = r; what = name; } };
    if (up) {
        step(ncclSend(top_own, row, ncclDouble, s->rank - 1, s->comm, c->stream), "ncclSend(up)");
        step(ncclRecv(top_halo, row, ncclDouble, s->rank - 1, s->comm, c->stream), "ncclRecv(up)");
    }
    if (dn) {
        step(ncclSend(bot_own, row, ncclDouble, s->rank + 1, s->comm, c->stream), "ncclSend(down)");
        step(ncclRecv(bot_halo, row, ncclDouble, s->rank + 1, s->comm, c->stream), "ncclRecv(down)");
    }
    const ncclResult_t end = ncclGroupEnd();
    if (first != ncclSuccess) return fail(DEFF_ECOMM, "%s failed: %s", what, ncclGetErrorString(first));
    if (end != ncclSuccess) return fail(DEFF_ECOMM, "ncclGroupEnd failed: %s", ncclGetErrorString(end));
    return DEFF_OK;
}

static int rank_gather(deff_slab_rank *s, int phase)
{
    deff_ctx *c = s->slab.c;
    const CgSlab &cg = s->slab.cg;
    if (s->gather) {
        s->h_cg_all.resize((size_t)(s->nranks + 1) * CG_SLAB_SLOT);
        double *mine = s->h_cg_all.data() + (size_t)s->nranks * CG_SLAB_SLOT;
        HIP_TRY(hipMemcpyAsync(mine, slcg_slot(cg, phase, s->rank), sizeof(double) * CG_SLAB_SLOT, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (s->gather(s->user, mine, s->h_cg_all.data(), (size_t)CG_SLAB_SLOT) != 0)
            return fail(DEFF_ECOMM, "custom all-gather of the CG sums failed");
        HIP_TRY(hipMemcpyAsync(slcg_slot(cg, phase, 0), s->h_cg_all.data(), sizeof(double) * CG_SLAB_SLOT * s->nranks,
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return DEFF_OK;
    }
    NCCL_TRY(ncclAllGather(slcg_slot(cg, phase, s->rank), slcg_slot(cg, phase, 0), (size_t)CG_SLAB_SLOT, ncclDouble, s->comm,
                           c->stream));
    return DEFF_OK;
}

static SlabSet cg_slabs_of(deff_slab_rank *s)
{
    SlabSet set = slabs_of(s);
    set.total = s->nranks;
    set.first = s->rank;
    set.send_row = [s](int, double *(*buf)(const Slab &)) { return rank_send_row(s, buf); };
    set.gather = [s](int, int phase) { return rank_gather(s, phase); };
    set.settle = [](int) { return DEFF_OK; };                    // a rank's sends are in its own stream's order
    return set;
}

// Collective, like deff_slab_rank_solve: every rank calls it with the same arguments and gets the same result.
extern "C" int deff_slab_rank_solve_cg(deff_slab_rank *s, double rtol, int64_t max_iter, int64_t check_every,
                                       deff_cg_result *out, double *MFL, double *MFR)
try {
    TRY(cg_arguments(s, out, rtol, max_iter, check_every));
    TRY(slab_solve_cg(cg_slabs_of(s), [s](double *deff_raw) { return rank_flux(s, deff_raw); }, rtol, max_iter, check_every,
                      out));
    if (MFL) memcpy(MFL, s->mfl.data(), sizeof(double) * s->NY);
    if (MFR) memcpy(MFR, s->mfr.data(), sizeof(double) * s->NY);
    return DEFF_OK;
}
DEFF_API_CATCH
