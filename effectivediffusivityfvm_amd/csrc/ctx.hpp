// ctx.hpp -- what the translation units of libdeff_amd.so share: the solver context, the error
// helpers, the internal entry points that cross files and the reference's stopping rule
// (JacobiCheck, check_step, deff_of_fluxes), which every Jacobi solve loop uses.
//   api_core.hip   library, context lifecycle, image, assembly (native / from D / imported), field
//   api_dict.hip   the row dictionary harvested from an explicit system
//   api_fill.hip   the flood fill on the device and the native 3-phase assembly on it (codes + a-priori row table)
//   api_sweep.hip  everything that plans or launches a sweep: the planner, the dealt tiles, the resident-launch
//                  protocol, the launchers, deff_sweeps; the streaming and single-sweep kernels
//   tiles_8wave.hip, tiles_tall.hip, tiles_12wave.hip
//                  the workgroup-tile kernels, one family each, listed for the planner (tile_kernels.hpp)
//   api_solve.hip  wall fluxes and the Jacobi solve loops (one image, batch, streaming batch); no sweep kernel
//   api_cg.hip     conjugate gradients to a residual tolerance (deff_solve_cg) and through refilled slots (deff_solve_cg_stream);
//                  every CG kernel, the slab forms included: their launches for one slab (cg_slab.hpp)
//   api_residual.hip  the reference's Residual() of the current field (deff_residual, deff_residual_slot, deff_residual_D)
//   api_facepass.hip  the five passes that are one walk over the faces (kernels_facepass.hpp) and the three side vectors they read:
//                  the Deff gradient (deff_sensitivity, deff_sensitivity_D), the field adjoint's (x, lambda, D) -> dL/dD
//                  (deff_field_vjp_D), the field tangent's right-hand side (deff_tangent_rhs_D) and lambda's own
//                  (deff_adjoint_tangent_rhs_D: k_tan on lambda), the Deff Hessian-vector product (deff_sensitivity_hvp_D), the
//                  field adjoint's second order (deff_field_vjp_hvp_D); one host path (face_pass_run) and one final kernel for
//                  the five; set / get / device pointer of lambda, dx and dlambda (SideVec below).  The solves that compute
//                  the three vectors are in api_cg.hip, beside the loop they run
//   api_flux.hip   the flux field: the pass (x, D) -> fx, fy, left and the section sums (deff_flux_field, deff_flux_field_D),
//                  kernels_flux.hpp
//   cell_pass.hpp  the host path those passes and the residual share (CellPass below): work-item planner, partial sums, the
//                  call's own event pair, the D plane (a caller's, or the assembled image's), the device-map getter; the final
//                  sums are one body (wave_reduce.hpp)
//   api_volume.hip 3-D volumes: deff_volume, a private context of nx x (ny * nz) plus the z-link planes (its kernels and its solve
//                  are in api_cg.hip, beside the plane form they extend: kernels_cg_volume.hpp)
//   api_slab.hip   one image over several GPUs: row slabs -- one slab type, pass loop and solve loop
//                  for both forms, which differ in the transport only (peer copies in one process,
//                  RCCL or a caller-supplied transport with one process per GPU); conjugate gradients over the slabs
//                  (slab_solve_cg: the loop and what travels between slabs)
// The library is built with -fvisibility=hidden; only the C ABI of include/deff_amd.h is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/deff_amd.h"
#pragma GCC visibility pop
#include "fvm_row.hpp"
#include "kernels_setup.hpp"
#include "lut_layout.hpp"

using namespace deff;

// ------------------------------------------------------------- errors -----

extern thread_local char g_err[512];                 // message of this thread's last failure (api_core.hip)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(e_ == hipErrorOutOfMemory ? DEFF_ENOMEM : DEFF_EHIP,             \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                       \
    } while (0)

#define TRY(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != DEFF_OK) return rc_; \
    } while (0)

// ------------------------------------------------------------ context -----

// What every pass over the cells keeps for its timed window and for deff_get_plan (cell_pass.hpp: cell_pass_start, pass_record).
struct PassPlan {
    bool have = false;              // the pass's maps hold a result
    // The call's own event pair, created by the first call that asks for `ms`: ev0 / ev1 of the context belong to the solve
    // loops alone, which read them at every check and may call a pass in between (a deff_set_progress or deff_image_done_fn
    // callback).
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int kt = 0;                     // tuning "res_kt" / "sens_kt" / "vjp_kt" / "tan_kt" / "hvp_kt" / "fhvp_kt" / "flux_kt": tiles of 8 rows a wave streams through (0 = planner)
    // deff_get_plan "*_kt" / "*_items" of the last call that launched: the run length used (planner, override and clip
    // applied) and the work items per image (the partial sums the final kernel adds)
    int plan_kt = 0, plan_items = 0;
};

// What one pass over the cells of the current field keeps between calls (the residual, the Deff gradient, the field adjoint's
// pass; cell_pass.hpp has what they do with it).
struct CellPass : PassPlan {
    double *map = nullptr;          // device: the last per-cell map (pitch nx), kept until the next call; the residual has none
    double *part = nullptr;         // device: the work items' partial sums + one sum per image, grow-only
    size_t part_cap = 0;
};

// What the flux-field pass keeps between calls (api_flux.hip, kernels_flux.hpp; cell_pass.hpp has its room and its release).
struct FluxPass : PassPlan {
    double *fx = nullptr, *fy = nullptr;    // device: the last face-flux maps (pitch nx), kept until the next call
    double *left = nullptr;                 // device: the left wall's flux per row of the stack
    double *colpart = nullptr, *wallpart = nullptr;   // device: the work items' column sums (pitch nx) and left-wall sums, grow-only
    size_t part_cap = 0;                    // chunks (images x work items per strip and image) the two hold
    double *Q = nullptr;                    // device: nimg x (nxt + 1) section sums
};

// A vector a side solve computes on the current matrix (api_cg.hip: side_solve) or a caller sets (api_facepass.hip:
// side_vec_set), both buffers allocated by the first call that needs them.  x: the solution (pitch nx, pad column 0); rhs: its
// right-hand side with the forward system's decoupled cells zeroed; rhs_ok: the pass map that is copied into rhs was computed
// since what the vector depends on was last replaced; valid: x belongs to it.  adjoint_reset / adjoint_tangent_reset below
// clear the two flags.
struct SideVec {
    double *x = nullptr, *rhs = nullptr;
    bool rhs_ok = false, valid = false;
};

struct deff_ctx {
    int device = 0;
    int nx = 0, ny = 0;             // mesh of ONE image
    int nimg = 1;                   // images stacked in this context (batch), see kernels_setup.hpp
    int rows = 0;                   // nimg * ny
    size_t n_img = 0;               // cells per image
    size_t n = 0;                   // cells in the stack
    double dx = 0, dy = 0;
    // nx is the width of every device array (even); nxt <= nx the width of the mesh -- an odd mesh
    // width is padded by one column of cells outside the mesh (kernels_setup.hpp, "Row pitch")
    int nxt = 0;
    // Row slab of a taller image (multi-GPU split of one image): the arrays hold
    // `halo` rows above and below the `own_h` rows this context updates; array row li is mesh row
    // li - dom_lo of a mesh_ny-row mesh.  Plain contexts: dom_lo = 0, mesh_ny = own_h = ny, halo = 0.
    bool slab = false;
    int dom_lo = 0, mesh_ny = 0, own_lo = 0, own_h = 0, halo = 0;
    // cells the default sweeps-per-pass is keyed on: 0 = this context's own n; for a slab a figure derived from
    // (nx, NY, number of slabs) alone, so that every slab / rank of one image plans the SAME T whatever its own
    // row count (slabs differ by one row; a different T per slab would desynchronise passes and exchanges)
    size_t tb_ref_cells = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // image (pixels as decoded, W x H, before mesh amplification)
    uint8_t *pix = nullptr;
    int W = 0, H = 0, ampX = 1, ampY = 1;
    bool have_image = false;

    // explicit SoA system
    double *a0 = nullptr, *c0 = nullptr, *aW = nullptr, *aE = nullptr, *aS = nullptr, *aN = nullptr,
           *b = nullptr;
    bool have_explicit = false;
    double c0_omega = NAN;          // omega the c0 plane was built for

    // matrix-free system: one 16-bit code per cell + the dictionary of distinct rows (lut_layout.hpp)
    uint16_t *code = nullptr;
    double *lut = nullptr;          // device tables [LUT_PLANES][LUT_PLANE_STRIDE]
    std::vector<double> lut_rows;   // host: rows [nrows][6] = A0, aW, aE, aS, aN, b (row 0 = zeros)
    int lut_nrows = 0;
    bool lut_allb = false;          // some row away from the walls has b != 0 (harvested dictionaries only)
    bool lut_guard = false;         // some c0 = w/A0 is not finite: the reference's non-zero link test matters
    bool have_matfree = false;
    bool dict_tried = false;        // a dictionary was already looked for in the current explicit system
    int dict_enabled = 1;
    // deff_get_plan "dict_outcome" / "dict_rows": how the harvest of the current explicit system ended -- 0 none tried, 1 harvested,
    // 2 more distinct rows than the table seats, 3 the hash table overflowed, 4 the verification pass found a mismatch -- and
    // the rows it found (the zero row not counted; 0 unless the outcome is 1).  Reset together with dict_tried (dict_reset).
    int dict_outcome = 0, dict_rows = 0;
    // an imported system (deff_set_system) with a non-zero W link in the first column or E link in the last:
    // the reference's kernel addresses neighbours linearly (x[p-1], x[p+1], cuh:80-83), so such a link reads the
    // neighbouring ROW's end cell.  Only the explicit / scalar kernels keep that addressing; the dictionary and the
    // temporally blocked kernel treat a wall column's outer neighbour as absent -- such a system stays explicit.
    bool wrap_links = false;
    double lut_omega = NAN;
    // Pre-scaled sweep arithmetic (kernels_sweep.hpp, pre_cell; tuning key "prescaled", opt-in): a second device table in the
    // dictionary's layout with aK' = (w/A0) aK in planes 1...4 and b' = (w/A0) b in plane 5 (plane 0 unused), built from lut_rows
    // by upload_lut_pre for one omega; upload_lut invalidates it whenever it rebuilds the dictionary's table.
    // lut_pre_allb: some row with b = 0 has a b' that is not +0.0 -- every strip then looks b' up.
    int prescaled = 0, plan_prescaled = 0;
    double *lut_pre = nullptr;
    double lut_pre_omega = NAN;
    bool lut_pre_allb = false;
    double Ds = 0, Df = 0;          // phase diffusivities of the native 2-phase system
    // what deff_residual() needs to know about a system assembled from the image: 2 / 3 pixel classes (0 = the system came
    // from a caller's D plane or matrix) and their diffusivities {fluid, solid, gas}
    int phase_mode = 0;
    double phase_D[3] = {0, 0, 0};

    // wall data for the flux evaluation
    double *Dl = nullptr, *Dr = nullptr;
    double CL = 0, CR = 0;
    bool have_walls = false;
    double *mf = nullptr;           // device: 2*ny fluxes
    double *mf_host = nullptr;      // pinned
    // where the fluxes are summed: 0 = on the host, in row order (default); 1 = on the device in the same order (bit-identical;
    // a check then moves 16 B per image instead of 16 B per row); 2 = on the device by a wave-level tree (fixed order, not the
    // reference's: ~1e-16 relative).  Row slabs always sum on the host (the rows of one image live on several devices).
    int flux_reduce = 0;
    double *q = nullptr;            // device: {Q1, Q2} per image
    double *q_host = nullptr;       // pinned
    bool q_valid = false;           // q_host holds the sums of the last flux_rows()

    // field, ping-pong
    double *x[2] = {nullptr, nullptr};
    int cur = 0;
    bool have_field = false;
    // batch bookkeeping: images still iterating (device mask is only bound while some are
    // frozen) and, per image, the ping-pong buffer that holds its newest field
    uint8_t *active = nullptr;
    std::vector<uint8_t> active_h, buf_of;
    bool masked = false;
    bool in_stream = false;         // inside deff_solve_stream: buf_of[] is current for every slot

    // scratch for chunked uploads (AoS import, D upload)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;

    deff_progress_fn progress = nullptr;
    void *progress_user = nullptr;

    int kernel = DEFF_KERNEL_AUTO;
    int rows_explicit = 0, rows_matfree = 0;     // rows per register tile, 0 = default
    int wg_matfree = 0;                          // persistent workgroups of the matrix-free kernel, 0 = default
    int nt_explicit = 1;                         // non-temporal coefficient loads in the explicit kernels
    int serpentine = 1;                          // alternate the tile walk direction from sweep to sweep
    int tb_T = 0, tb_LY = 0, tb_wg = 0;          // temporal blocking: sweeps per pass, rows per chunk, workgroups
    unsigned long long *tb_stamps = nullptr;     // diagnostics: per wave-tile start/end clocks (deff_debug_tb_stamps)
    int tb_wall_halo = 2;                        // strip placement: 1 = halo also outside the walls, 0 = not, 2 = whichever needs fewer strips
    int plan_T = 0, plan_LY = 0, plan_ntx = 0, plan_cpi = 0, plan_blocks = 0;   // last temporally blocked plan
    int plan_impl = 0, plan_R = 0, plan_NW = 0;
    // form of a temporally blocked pass: 0 = chosen by the planner, 1 = streaming (kernels_tb.hpp: one wave per tile),
    // 2 = workgroup tiles (kernels_wgtile.hpp: 8 waves per tile, rows resident in registers); tb_R = rows per wave there
    int tb_impl = 0, tb_R = 0, tb_NW = 0;
    // resident passes (kernels_wgtile.hpp, k_sweep_wgres): when every tile of the context is on the chip at once, all the
    // passes between two checks are ONE launch whose tiles keep their matrix rows and owned cells in registers and wait
    // for their neighbours only.  Tuning key "tb_launch": 0 = resident passes whenever the tiles are co-resident (default:
    // the grid fits the chip by the occupancy query, resident launches of one process are chained per device,
    // api_sweep.hip, so that two of them never share the chip, and every wait is bounded); 1 = never (one launch per pass).
    // What the process cannot rule out -- another PROCESS on the same GPU, a CU mask -- ends in a bounded wait running
    // out; the solve then restores the field it had when the interval's first resident launch was enqueued, redoes the
    // interval with one launch per pass and stays in that mode (res_fallbacks counts these; deff_get_plan "tb_fallbacks").
    int tb_resident = 1;
    // is the matrix-free system link-symmetric (k_links_symmetric)?  0 = not looked at since the codes / dictionary last
    // changed, 1 = yes (tall tiles then do 7 lookups per row instead of 10), 2 = no
    int links_sym = 0;
    int tb_sym = 0;                              // tuning: 2 = never use the symmetric short-cut (A/B, tests)
    int tb_debug_stall = 0;                      // tests: tile (index + 1) that leaves a resident launch without publishing
    int tb_debug_stall_skip = 0;                 // tests: ... after this many further resident launches
    int plan_resident = 0;                       // the last plan used resident passes
    unsigned *res_flags = nullptr;               // per tile: passes completed (epoch counter)
    size_t res_flags_n = 0;
    unsigned res_epoch = 0;
    unsigned *res_abort = nullptr;               // raised by a workgroup whose wait for a neighbour ran out
    bool res_pending = false;                    // a resident launch was enqueued since the flag was last read
    // restart point of the resident launches in flight: a copy of x[res_backup_cur] taken in front of the first resident
    // launch after a synchronised look at the abort flag, and the sweeps enqueued since (with their omega)
    double *res_backup = nullptr;
    int res_backup_cur = 0;
    int64_t res_redo = 0;
    double res_omega = 0;
    int res_fallbacks = 0;                       // aborted resident intervals redone with one launch per pass
    bool chain_counted = false;                  // this context is counted among its device's users of the resident chain's event
    int fma = 0;                                 // contracted arithmetic (kernels_sweep.hpp), opt-in
    int tb_xmajor = 1;                           // wave-tile numbering of the temporally blocked kernel
    // Streaming kernel, chunk heights by service order (deal_ranked_tiles, api_sweep.hip): 0 = equal chunks, 1 = dealt tiles.
    // tb_rank_w: the relative speed (per mille) of a SIMD's oldest / second / youngest wave, tb_rank_wall: what a row of a wall strip
    // costs, per mille of an inner strip's (its waves look up b as well)
    int tb_tall_deal = 1;                        // tall tiles: rows dealt by the waves' age where a kernel for it exists (tiles_tall.hip)
    int plan_aged = 0;
    int tb_sym_age = 1;                          // 12-wave tiles: the shapes with a row less for the youngest waves (tiles_12wave.hip)
    int tb_sym_shape = 0;                        // tests: 1-based index into the 12-wave shapes of T = 8 in TILES_12WAVE (0: the planner's choice)
    int tb_ranked = 1;
    int tb_rank_w[3] = {460, 325, 215};
    int tb_rank_wall = 1100;
    int4 *tb_dealt = nullptr;                    // device table: (strip, first row, rows, stamp index) per wave of the grid
    size_t tb_dealt_cap = 0;
    std::vector<int4> tb_dealt_host;
    std::vector<int> tb_dealt_key;               // what the table was built for
    size_t tb_dealt_miss_at = 0;                 // index of the table's last element: the waves' count of misplacements
    int64_t tb_dealt_waves = 0;                  // waves launched on the current table
    int tb_dealt_looks = 0;                      // times the count was read (dealt_watch: the first three synchronisations)
    int tb_rank_misses = 0, tb_rank_lost = 0;    // last count read; 1 = the dispatch order is not the assumed one: equal chunks from now on
    int tb_dealt_min = 0, tb_dealt_max = 0;      // rows of the shortest and of the tallest chunk of the table ("tb_chunk_min", "tb_chunk_max")
    int tb_dealt_LY = 0, tb_dealt_nmax = 0;      // ... and what deff_get_plan reports of it (an inner strip's middle rank; most chunks per rank)
    int plan_ranked = 0;
    // Chained streaming passes (k_sweep_matfree_tb_chain, kernels_tb.hpp): the passes between two checks as ONE launch of the
    // dealt tiles, each tile waiting only for its neighbours (tb_chain.hpp).  Tuning key "tb_chain": 0 = one launch per pass.
    // Runs through the resident launches' machinery: flags, restart copy, abort word, fallback (which clears tb_resident).
    int tb_chain = 1;
    int plan_chain = 0;                          // the last plan chained its passes
    unsigned *tb_chain_nbrs = nullptr;           // device: TB_CHAIN_MAXN neighbour slots (+ 1; 0 = none) per entry of tb_dealt
    size_t tb_chain_nbrs_cap = 0;
    bool tb_chain_fits = false;                  // the current table's lists fit (else it is not chained)
    int64_t last_launches = 0;                   // sweep-kernel launches of the last deff_sweeps()/deff_solve()

    // conjugate gradients (api_cg.hip): work vectors, CG table, per-image scalars and the loop's own event pair, allocated
    // by the first deff_solve_cg
    double *cg_r = nullptr, *cg_p[2] = {nullptr, nullptr};
    double *cg_tab = nullptr;                    // device table [CG_PLANES][LUT_PLANE_STRIDE] (kernels_cg.hpp)
    double *cg_part = nullptr;                   // partial sums, 3 per work item
    size_t cg_part_cap = 0;
    void *cg_scal = nullptr;                     // CgScal per image
    unsigned *cg_flags = nullptr;                // [0] admissibility, [1] images restarted by a true-residual round
    hipEvent_t cg_ev0 = nullptr, cg_ev1 = nullptr;
    int cg_plan_kr = 0, cg_plan_ntx = 0, cg_plan_items = 0;   // deff_get_plan "cg_kr" / "cg_strips" / "cg_items" of the last deff_solve_cg
    int cg_plan_restarts = 0;                    // ... and its true-residual rounds that restarted an image ("cg_restarts")
    // tuning "cg_onchip": 1 = images of at most 16 384 cells (pitch x ny) iterate on one compute unit each (kernels_cg_image.hpp);
    // 0 (default) = the streaming kernels for every size.  cg_plan_impl: what the last deff_solve_cg ran, 1 streaming, 2 on chip
    int cg_onchip = 0, cg_plan_impl = 0;
    int cg_cus = 0;                              // compute units of the device (workgroups of an on-chip launch)
    // tuning "cg_planes": deff_solve_cg on the explicit coefficient planes (kernels_cg_planes.hpp; cg_plan_impl 3) -- 1 = for a
    // system that has no row dictionary, 2 = for every system (tests: the bits are the table form's); 0 (default) = never.
    // cg_inv (1 / a0 per cell, 0 on decoupled cells) and cg_q (A p) are allocated by the first call that takes that form
    int cg_planes = 0;
    // tuning "cg_onchip_planes": 1 = a solve on the coefficient planes (deff_solve_cg where it takes that form, and the side
    // solves deff_solve_adjoint / _tangent / _adjoint_tangent) iterates images of at most 16 384 cells on one compute unit each
    // (kernels_cg_image_planes.hpp; cg_plan_impl 4); 0 (default) = the streaming plane kernels for every size
    int cg_onchip_planes = 0;
    double *cg_inv = nullptr, *cg_q = nullptr;
    // tuning "cg_fold": 1 = an iteration of the streaming forms is two launches, the image's last workgroup to arrive does what
    // k_cg_alpha / k_cg_beta do (kernels_cg_fold.hpp); 2 = as 1, the table form's direction kernel with loads a row ahead;
    // 0 (default) = four launches.  cg_plan_fold: what the last CG call ran.  cg_tick: the arrival counters of the two folded
    // launches, per image its own and one per shard of items (kernels_cg_fold.hpp)
    int cg_fold = 0, cg_plan_fold = 0;
    unsigned *cg_tick = nullptr;
    size_t cg_tick_cap = 0;
    // deff_solve_cg_stream (api_cg.hip, kernels_cg_stream.hpp), allocated by the first one.  cgs_dev: the round's slot list,
    // the slots' restart rounds, and the staging area -- the entering slots' list followed by their pixels --; cgs_pin: the
    // pinned mirror of the two lists and the pixels, two snapshots of the slots' CgScal + flags, and a round's results
    void *cgs_dev = nullptr, *cgs_pin = nullptr;
    size_t cgs_dev_bytes = 0, cgs_pin_bytes = 0;
    hipEvent_t cgs_ev[2] = {nullptr, nullptr};   // a snapshot has arrived
    int cgs_intervals = 0, cgs_launches = 0, cgs_waits = 0;   // deff_get_plan: figures of the last stream

    // The passes over the cells of the current field (cell_pass.hpp), everything allocated by the first call that needs it:
    //   pass_res   deff_residual / deff_residual_slot / deff_residual_D (api_residual.hip): no map; plan_kt is 0 after deff_residual_D
    //   pass_sens  deff_sensitivity / deff_sensitivity_D (api_facepass.hip, like the next five): the map dDeff/dD, handed out by deff_device_sensitivity
    //   pass_vjp   deff_field_vjp_D: the map dL/dD, handed out by deff_device_field_vjp
    //   pass_tan   deff_tangent_rhs_D: the map r = db - dA x, handed out by deff_device_tangent_rhs
    //   pass_hvp   deff_sensitivity_hvp_D: the map H dD, handed out by deff_device_sensitivity_hvp
    //   pass_atan  deff_adjoint_tangent_rhs_D: the map q = -dA lambda, k_tan's on lambda; a map of its own, so
    //              that pass_tan's stays
    //   pass_fhvp  deff_field_vjp_hvp_D: the map S_w dD, handed out by deff_device_field_vjp_hvp
    CellPass pass_res, pass_sens, pass_vjp, pass_tan, pass_hvp, pass_atan, pass_fhvp;
    //   pass_flux  deff_flux_field / deff_flux_field_D (api_flux.hip): the maps fx, fy, handed out by deff_device_flux_field
    FluxPass pass_flux;
    bool grid_given = false;        // the last deff_assemble_3phase was given a Grid (deff_sensitivity refuses such a system)

    // The side vectors (api_facepass.hip; their solves are api_cg.hip's loop), each for the current system and image:
    //   adj   lambda of A lambda = w, w the caller's dL/dx (deff_solve_adjoint / deff_set_adjoint); rhs_ok is not used
    //   tan   dx of A dx = r, r pass_tan's map (deff_solve_tangent / deff_set_tangent); deff_sensitivity_hvp_D reads it
    //   atan  dlambda of A dlambda = q, q pass_atan's map (deff_solve_adjoint_tangent / deff_set_adjoint_tangent); for the
    //         current lambda too: every call that replaces lambda resets it
    SideVec adj, tan, atan;

    // Native 3-phase system (kernels_fill.hpp, api_fill.hip): the flood fill of the pore space as bitmaps -- one `open` and
    // one `reach` word per 64 columns of a row, fill_nw words per row --, its status words and the tiled form's `changed` words.
    // fill_valid: reach is the fill of the current pixels (image_shape clears it: every new image goes through there);
    // codes3_valid: code[] holds the native 3-phase codes of that fill (cleared by whoever else writes code[]);
    // native3: the current system is the native 3-phase one (its explicit planes are built on demand, explicit_from_image)
    uint64_t *fill_open = nullptr, *fill_reach = nullptr;
    int *fill_status = nullptr;
    unsigned *fill_changed = nullptr;
    int fill_nw = 0;
    bool fill_valid = false, codes3_valid = false, native3 = false;
    std::vector<int> fill_path;                  // PathFlag per image
    unsigned rows3_used[16] = {};                // bit k: some cell of the current image has table row k (k_phase_codes3)
    int fill_impl = 0, fill_tile_rows = 0;       // tuning: form (0 = by size, 1 = one workgroup per image, 2 = tiles), rows per tile
    // deff_get_plan: form and launches of the last fill, fills computed and images handed to the host fill since creation
    int fill_plan_impl = 0, fill_plan_launches = 0, fill_runs = 0, fill_fallbacks = 0;
    int fill_plan_rounds = 0;                    // most rounds a workgroup of the last fill took ("fill_rounds")
};

static inline int use_device(const deff_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    return DEFF_OK;
}

template <typename T>
static inline int dev_alloc(T **p, size_t count)
{
    if (*p) return DEFF_OK;
    HIP_TRY(hipMalloc((void **)p, count * sizeof(T)));
    return DEFF_OK;
}

static inline int ensure_scratch(deff_ctx *c, size_t bytes)
{
    if (c->scratch_bytes >= bytes) return DEFF_OK;
    if (c->scratch) { HIP_TRY(hipFree(c->scratch)); c->scratch = nullptr; c->scratch_bytes = 0; }
    HIP_TRY(hipMalloc(&c->scratch, bytes));
    c->scratch_bytes = bytes;
    return DEFF_OK;
}

static inline int ensure_explicit(deff_ctx *c)
{
    TRY(dev_alloc(&c->a0, c->n)); TRY(dev_alloc(&c->c0, c->n));
    TRY(dev_alloc(&c->aW, c->n)); TRY(dev_alloc(&c->aE, c->n));
    TRY(dev_alloc(&c->aS, c->n)); TRY(dev_alloc(&c->aN, c->n));
    TRY(dev_alloc(&c->b, c->n));
    return DEFF_OK;
}

static inline int ensure_walls(deff_ctx *c)
{
    TRY(dev_alloc(&c->Dl, (size_t)c->rows));
    TRY(dev_alloc(&c->Dr, (size_t)c->rows));
    TRY(dev_alloc(&c->mf, (size_t)2 * c->rows));
    if (!c->mf_host) HIP_TRY(hipHostMalloc((void **)&c->mf_host, sizeof(double) * 2 * c->rows));
    return DEFF_OK;
}

static inline int grid_for(size_t n, int cap = 16384)
{
    size_t g = (n + 255) / 256;
    return (int)(g < (size_t)cap ? (g ? g : 1) : (size_t)cap);
}

// rows of nxt elements on the host <-> rows of nx elements on the device
template <typename T>
static inline int rows_h2d(deff_ctx *c, T *dst, const T *src, size_t rows)
{
    if (c->nx == c->nxt)
        HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * c->nx * rows, hipMemcpyHostToDevice, c->stream));
    else
        HIP_TRY(hipMemcpy2DAsync(dst, sizeof(T) * c->nx, src, sizeof(T) * c->nxt, sizeof(T) * c->nxt, rows,
                                 hipMemcpyHostToDevice, c->stream));
    return DEFF_OK;
}
template <typename T>
static inline int rows_d2h(deff_ctx *c, T *dst, const T *src, size_t rows)
{
    if (c->nx == c->nxt)
        HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * c->nx * rows, hipMemcpyDeviceToHost, c->stream));
    else
        HIP_TRY(hipMemcpy2DAsync(dst, sizeof(T) * c->nxt, src, sizeof(T) * c->nx, sizeof(T) * c->nxt, rows,
                                 hipMemcpyDeviceToHost, c->stream));
    return DEFF_OK;
}

// a plane of the stack (true width on the host) into a device plane of pitch nx, the pad column zeroed
static inline int plane_h2d(deff_ctx *c, double *dst, const double *src)
{
    if (c->nx != c->nxt) HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * c->n, c->stream));
    return rows_h2d(c, dst, src, (size_t)c->rows);
}

static inline CoefSoA soa_of(deff_ctx *c) { return CoefSoA{c->a0, c->aW, c->aE, c->aS, c->aN, c->b}; }

// a new system: no dictionary was looked for in it yet
static inline void dict_reset(deff_ctx *c) { c->dict_tried = false; c->dict_outcome = 0; c->dict_rows = 0; }

// The only places that invalidate a side vector.  A new system or image: lambda, dx and the map that was dx's right-hand
// side were the old one's (their getters, passes and deff_solve_tangent: DEFF_ESTATE), and so was dlambda; a new lambda:
// dlambda and its right-hand side belonged to the old one.
static inline void side_vec_reset(SideVec &v) { v.rhs_ok = false; v.valid = false; }
static inline void adjoint_tangent_reset(deff_ctx *c) { side_vec_reset(c->atan); }
static inline void adjoint_reset(deff_ctx *c) { side_vec_reset(c->adj); side_vec_reset(c->tan); adjoint_tangent_reset(c); }

// The refusal of every entry point that needs all rows of the image on one device.
static inline int slab_refused(const deff_ctx *c, const char *who)
{
    if (c->slab) return fail(DEFF_EINVAL, "%s: not for row-slab contexts (the rows of the image live on several devices)", who);
    return DEFF_OK;
}

// No C++ exception may unwind through the C ABI: every `extern "C" int` entry point is a
// function-try-block ending in DEFF_API_CATCH, which turns std::bad_alloc (host vectors sized by the
// caller's image) and anything else into an error code + message.
static inline int api_exception() noexcept
{
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return fail(DEFF_ENOMEM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(DEFF_EINVAL, "internal error: %s", e.what());
    } catch (...) {
        return fail(DEFF_EINVAL, "internal error: unknown exception");
    }
}
#define DEFF_API_CATCH catch (...) { return api_exception(); }

// ------------------------------------------------- shared internals -------

struct TileKernel;
struct SweepPlan {
    int kernel = 0;
    double omw = 0;
    int rows = 0, cpi = 0, gx = 0, gy = 0, blocks = 0;   // single-sweep kernels (cpi: row tiles per image)
    // temporally blocked kernel
    bool fma = false;
    bool pre = false;                                     // the pre-scaled arithmetic (tuning "prescaled"): matrix-free family only
    int T = 0, LY = 0, tcpi = 0, ntx = 0, tgx = 0, tgy = 0, tblocks = 0;
    int shift = 0;                                        // column shift of the strips (0: no halo outside the walls)
    int T_override = 0;                                   // slab mode plans a T = 1 pass for remainders
    bool guard = false;                                   // streaming kernel: the reference's non-zero link test
    double omega = 0;                                     // as given to plan_sweeps (omw = 1 - omega)
    int impl = 1;                                         // 1 = streaming kernel, 2 = workgroup tiles
    const TileKernel *tile = nullptr;                     // impl 2: the tile's kernels, waves and rows (tile_kernels.hpp)
    const int4 *dealt = nullptr;                          // streaming kernel: dealt tiles (chunk heights by service order), or none
    bool resident = false;                                // impl 2 only: all passes of a batch in one launch (k_sweep_wgres)
    bool chained = false;                                 // impl 1, dealt tiles: all passes of a batch in one launch (k_sweep_matfree_tb_chain)
    const unsigned *nbrs = nullptr;                       //   ... and the tiles' neighbour lists
    // rows the plan updates: band_h > 0 restricts it to the band [band_lo, band_lo + band_h) of the context's owned rows
    // (input); own_lo / own_h are what the planner resolved (output, passed to the kernels)
    int band_lo = 0, band_h = 0, own_lo = 0, own_h = 0;
};

// The reference's stopping rule (JacobiGPU): Deff is evaluated at every check, and the loop goes on while its relative
// change since the previous check exceeds tol.  One per image of deff_solve_batch, per slot of deff_solve_stream and per
// row-slab solve.
struct JacobiCheck {
    double deffNew = 1, deffOld = 5, change = 100.0, conv = 0;      // cuh:1171-1173
    int64_t checks = 0;
    void update(double deff)
    {
        deffNew = deff;
        change = (deffOld - deffNew) / (deffOld);                   // cuh:1265
        deffOld = deffNew;
        conv = change;                                              // cuh:1275
        ++checks;
    }
    bool more(double tol) const { return tol < fabs(change); }     // cuh:1232
    // deff_raw: the value at the last check (cuh:1309)
    deff_result result(int64_t iters, float loop_ms) const { return deff_result{iters, checks, deffNew, conv, loop_ms}; }
};

// The sweeps from `iter` up to and including the next check -- the sweep with 0-based index k is followed by a check iff
// k % check_every == 0 (cuh:1243) -- or, when no check comes before max_iter, up to max_iter.
struct CheckStep {
    int64_t next_check, sweeps;
    bool check;
};
static inline CheckStep check_step(int64_t iter, int64_t max_iter, int64_t check_every)
{
    const int64_t next_check = ((iter + check_every - 1) / check_every) * check_every;
    const bool check = next_check < max_iter;
    return CheckStep{next_check, check ? next_check - iter + 1 : max_iter - iter, check};
}

// Deff from the wall fluxes of an image's ny rows, summed on the host in row order like the reference (cuh:1258-1263).
static inline double deff_of_fluxes(const double *L, const double *R, int ny, double CL, double CR)
{
    double Q1 = 0, Q2 = 0;
    for (int j = 0; j < ny; ++j) {
        Q1 += L[j];
        Q2 += R[j];
    }
    const double qAvg = (Q1 + Q2) / (2.0 * ny);
    return qAvg / ((CR - CL));
}

// api_core.hip
void reset_batch_state(deff_ctx *c);
int resolve_kernel(const deff_ctx *c, int *k);
int image_shape(deff_ctx *c, int W, int H, int ampX, int ampY);
void native2_rows(const deff_ctx *c, double Ds, double Df, double CL, double CR, std::vector<double> &rows);   // changes nothing
void commit_lut_rows(deff_ctx *c, std::vector<double> &rows);
void build_lut_rows(deff_ctx *c, double Ds, double Df, double CL, double CR);                                // both of them
int upload_lut(deff_ctx *c, double omega);
int upload_lut_pre(deff_ctx *c, double omega);           // after upload_lut(c, omega), on a table without a singular row
int consolidate(deff_ctx *c);
int explicit_from_image(deff_ctx *c);
// api_fill.hip
int native3_explicit(deff_ctx *c);                       // explicit planes of the native 3-phase system
// api_dict.hip
int ensure_dictionary(deff_ctx *c);                      // harvest the row dictionary of an explicit system, if allowed
// api_sweep.hip
int default_tb_T(const deff_ctx *c);
int clamp_tb_T(int T);
int default_tb_impl(const deff_ctx *c);
int plan_sweeps(deff_ctx *c, double omega, SweepPlan *pl);
// a stream has put new images into slots: plan again, or verify again, what the plan took from the old codes
int replan_for_new_codes(deff_ctx *c, double omega, SweepPlan *pl);
void enqueue_sweep(deff_ctx *c, const SweepPlan &pl);
int enqueue_tb_pass(deff_ctx *c, const SweepPlan &pl);
int launch_tb_pass(deff_ctx *c, const SweepPlan &pl);    // the same launch without flipping x[cur]
int dealt_watch(deff_ctx *c);                            // after a synchronisation: is the dispatch order the dealt tiles assume?
int enqueue_sweeps(deff_ctx *c, const SweepPlan &pl, int64_t n);   // stops at the first launch that fails
// did a resident launch give up waiting?  (synchronises if one is pending; on an abort the interval is redone with one
// launch per pass and the context stays in that mode)
int resident_check(deff_ctx *c);
void resident_chain_ctx_created(int device);
void resident_chain_ctx_destroyed(int device);
// api_solve.hip
int flux_rows(deff_ctx *c, bool need_rows = true);
// api_cg.hip: what a deff_volume (api_volume.hip) runs on its private context of nx x (ny * nz)
int volume_assemble_planes(deff_ctx *c, const double *dD, int ny, int nz, double dy, double dz, double CL, double CR, double *aB,
                           double *aF);
int volume_solve_cg(deff_ctx *c, const double *aB, const double *aF, int ny, double rtol, int64_t max_iter, int64_t check_every,
                    deff_cg_result *out, double *MFL, double *MFR);
// api_facepass.hip: the Deff gradient of a volume's field (k_sens3) into the private context's pass_sens; ny, dy, dz are the volume's
int volume_sens_run(deff_ctx *c, const double *D, int ny, double dy, double dz, double CL, double CR, double *g, double *euler,
                    float *ms);
