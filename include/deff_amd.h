/*
 * deff_amd.h -- C ABI of the MI355X-native effective-diffusivity hot path.
 *
 * One shared library, libdeff_amd.so (HIP, gfx950).  Plain pointers and sizes
 * only; no C++ or torch types cross this boundary.  The reference has no FFI:
 * its seam is function-level inside one translation unit, so
 * each entry point below cites the reference function (Deff2DGPU/Deff2D.cuh,
 * "cuh:line") whose work it takes over.  A C++ mirror with the reference's
 * own names and argument lists (DiscretizeMatrix2D, initializeGPU, JacobiGPU,
 * ...) sits on top of this ABI in
 * effectivediffusivityfvm_amd/csrc/reference_seam.hpp; see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns DEFF_OK (0) or a negative DEFF_E* code and never
 *     blocks on stdin (the reference calls getchar() on failure, cuh:912-916);
 *     deff_last_error() gives the message of the calling thread's last failure;
 *   - a context is bound to one device and one (nx, ny) mesh, owns every device
 *     buffer and one HIP stream, and is reused across images (the reference
 *     re-allocates and resets the device per image, cuh:2038, cuh:1015);
 *   - a context is not thread-safe; use one per host thread / per GPU;
 *   - host arrays are row-major, cell p = i*nx + j, exactly as in the
 *     reference; "AoS" coefficient arrays are [n][5] = P,W,E,S(row+1),N(row-1).
 */
#ifndef DEFF_AMD_H
#define DEFF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEFF_OK            0
#define DEFF_EINVAL       -1   /* bad argument / call order */
#define DEFF_EHIP         -2   /* a HIP runtime call failed */
#define DEFF_ENOMEM       -3   /* device or host allocation failed */
#define DEFF_ENODEV       -4   /* no usable gfx950 device */
#define DEFF_ESTATE       -5   /* system / field not set before solve */
#define DEFF_ECOMM        -6   /* RCCL failure (row-slab mode) */

/* sweep kernel selection, deff_set_kernel() */
#define DEFF_KERNEL_AUTO       0
#define DEFF_KERNEL_EXPLICIT   1   /* SoA coefficient streams, 64 B/cell/sweep */
#define DEFF_KERNEL_SCALAR     2   /* 1 cell/thread, any nx; correctness fallback */
#define DEFF_KERNEL_MATFREE    3   /* rows from the dictionary by a 16-bit code, 18 B/cell/sweep */
#define DEFF_KERNEL_MATFREE_TB 4   /* matrix-free, several sweeps per HBM pass */

typedef struct deff_ctx deff_ctx;

typedef struct deff_result {
    int64_t iters;      /* sweeps executed: 10000k+1 or max_iter (cuh:1289, return value) */
    int64_t checks;     /* convergence checks performed */
    double  deff_raw;   /* Deff at the LAST CHECK, not normalised by Df (cuh:1309) */
    double  conv;       /* last signed relative change (cuh:1275) */
    double  loop_ms;    /* hipEvent time of the sweep loop, same window as cuh:1230-1298 */
} deff_result;

/* ---- library ---------------------------------------------------------- */
const char *deff_version(void);
const char *deff_last_error(void);
const char *deff_error_string(int code);
int deff_device_count(int *count);

/* ---- lifecycle: replaces initializeGPU cuh:904-981 / unInitializeGPU cuh:983-1021 */
int deff_create(int device, int nx, int ny, deff_ctx **out);
/* dataset-generation mode (BatchSim cuh:1843-2054): `nimg` images of the same nx x ny mesh are
 * held and swept together as one stacked domain (image k = rows [k*ny, (k+1)*ny)); every
 * array argument of the calls below then covers the whole stack, image after image.  The
 * zero-flux top/bottom boundaries keep the images uncoupled, so each image's numbers are
 * those of a one-at-a-time run. */
int deff_create_batch(int device, int nx, int ny, int nimg, deff_ctx **out);
int deff_batch_size(const deff_ctx *ctx, int *nimg);
/* how many slots a stack context for `images` images of an nx x ny mesh should have on `device` (dataset generation:
 * small images that fit one workgroup tile get one slot per CU and stay resident; otherwise ~16-64 Mi cells per stack) */
int deff_recommended_batch(int device, int nx, int ny, int64_t images, int *slots);
int deff_destroy(deff_ctx *ctx);
int deff_mesh(const deff_ctx *ctx, int *nx, int *ny, double *dx, double *dy);   /* meshInfo cuh:54-61 */
int deff_set_kernel(deff_ctx *ctx, int kernel);
int deff_get_kernel(const deff_ctx *ctx, int *kernel_in_use);
/* tuning knob; 0 restores the default.  Keys: "rows_explicit", "rows_matfree", "wg_matfree",
 * "nt_explicit", "serpentine", "tb_T" (sweeps per pass: 1,2,4,6,8), "tb_LY" (rows per chunk), "tb_wg",
 * "tb_xmajor", "tb_wall_halo", "tb_ranked" (streaming kernel: chunk heights by the service order of a SIMD's waves, 1 default;
 * weights "tb_rank_w0", "tb_rank_w1", "tb_rank_w2", "tb_rank_wall" per mille), "tb_chain" (streaming kernel on dealt tiles: 1 default =
 * the passes between two checks run as ONE launch, every tile waiting only for the tiles whose rows it reads or overwrites, under the
 * rules of "tb_launch" below, fallback included; 0 = one launch per pass; deff_get_plan "tb_chain"), "tb_tall_deal" / "tb_sym_age" (resident tiles: rows
 * dealt by the waves' age, 1 default), "dict" (harvest a row dictionary from explicit systems: 1 default),
 * "tb_impl" (1 streaming, 2 workgroup tiles), "tb_R", "tb_NW" (8 / 12 / 16 waves per
 *   tile: 12 = link-symmetric matrix rows in registers, 16 = tall resident tiles),
 * "cg_onchip" (deff_solve_cg: 1 = images of at most 16 384 cells iterate on one compute unit each, see there),
 * "cg_planes" (deff_solve_cg on the explicit coefficient planes: 1 = for a system without a row dictionary, 2 = always;
 *   values above 2 are DEFF_EINVAL; see there),
 * "cg_onchip_planes" (CG solves on the coefficient planes -- deff_solve_cg where it takes that form, deff_solve_adjoint,
 *   deff_solve_tangent, deff_solve_adjoint_tangent: 1 = images of at most 16 384 cells iterate on one compute unit each; values
 *   above 1 are DEFF_EINVAL; see deff_solve_cg),
 * "cg_fold" (deff_solve_cg / deff_solve_cg_stream: 1 = two launches per iteration instead of four, 2 = as 1 with loads a row
 *   ahead; values above 2 are DEFF_EINVAL; see deff_solve_cg),
 * "fill_impl" (deff_assemble_3phase_native: form of the flood fill on the device, 0 = by size, 1 = one workgroup per image,
 *   2 = row tiles over several launches; values above 2 are DEFF_EINVAL, 1 on an image whose bitmaps do not fit one
 *   workgroup is DEFF_EINVAL at the assembly) and "fill_tile_rows" (rows per tile of form 2, 0 = the planner's choice; clipped
 *   to the image and to what fits a workgroup) -- both exist so that the tiled form and its seams can be tested at small shapes,
 * "res_kt" (deff_residual / deff_residual_slot: tiles of 8 rows one wave streams through, a "run"; 0 = the planner's choice,
 *   about 4 096 work items per launch; clipped to the image's tile rows; deff_get_plan "res_kt"),
 * "sens_kt" (deff_sensitivity / deff_sensitivity_D: the same for the gradient pass; deff_get_plan "sens_kt"),
 * "vjp_kt" (deff_field_vjp_D: the same for the field adjoint's pass; deff_get_plan "vjp_kt"),
 * "tan_kt" (deff_tangent_rhs_D: the same for the field tangent's pass; deff_get_plan "tan_kt"),
 * "hvp_kt" (deff_sensitivity_hvp_D: the same for the Hessian-vector pass; deff_get_plan "hvp_kt"),
 * "fhvp_kt" (deff_field_vjp_hvp_D: the same for the field adjoint's second-order pass; deff_get_plan "fhvp_kt"),
 * "flux_kt" (deff_flux_field / deff_flux_field_D: the same for the flux-field pass, where it also fixes the order of the
 *   section sums; deff_get_plan "flux_kt"),
 * "tb_launch" (workgroup tiles whose tiles all fit the chip
 *   run every pass between two checks in ONE launch, neighbouring tiles synchronised by flags: 1 = one launch per
 *   pass instead; a resident launch that cannot make progress -- another process holds part of the GPU -- gives up
 *   after a bounded wait, the interval is redone with one launch per pass and the context stays in that mode:
 *   deff_get_plan "tb_fallbacks"), "flux_reduce", and
 *   "fma" = 1: contracted arithmetic -- the reference's expressions (cuh:74-89, cuh:1957) with each
 *   product fused into the following add, as nvcc's default -fmad=true / gcc -ffp-contract=fast compile
 *   them; bit-identical to the oracle's fma build, not to the default (written-order) arithmetic.
 *   Set it before deff_init_linear(); it applies to every sweep kernel.
 *   "prescaled" = 1 (0 restores the default; values above 1 are DEFF_EINVAL): pre-scaled sweep arithmetic, opt-in.  The row
 *   dictionary is scaled once per table row on the host, aK' = (w/A0) aK and b' = (w/A0) b (one rounded product each), and a
 *   cell of a sweep is five dependent FMAs,
 *       acc = fma(1 - w, xC, b'); acc = fma(-aW', xW, acc); ... E, S ...; xNew = fma(-aN', xN, acc),
 *   every term evaluated, neighbours outside the mesh read as +0.0: 5 FP64 instructions and 5 lookups per cell instead of
 *   11 and 6.  NOT the reference's written operation order: results agree with the default to ~1e-13 (field rel-L2, Deff),
 *   with the same iteration counts on the recorded configurations, and are never bit-identical to it.  Applies to
 *   deff_sweeps, deff_solve, deff_solve_batch and deff_solve_stream on plain and stacked contexts; flux, residual and CG
 *   are untouched; "fma" is ignored by the sweeps while it is set (and still governs deff_init_linear).  Matrix-free
 *   kernels only: blocked passes take the streaming form at every size, one launch per pass (never chained or resident;
 *   "tb_T", "tb_LY", "tb_ranked", "tb_xmajor", "wg_matfree" keep working).  The workgroup-tile, resident, chained, explicit
 *   and scalar forms have no pre-scaled variant: below ~4 Mi cells the default arithmetic on resident tiles may well stay
 *   faster.  Refused with DEFF_EINVAL at the call that would sweep (field, system and plan stay as they were): a system
 *   without a row dictionary, a context set to DEFF_KERNEL_EXPLICIT / _SCALAR, a dictionary with a singular row (a phase
 *   with D = 0 and no ImpSolid rows: w/A0 is not finite).  Row-slab contexts refuse the key itself.
 *   deff_get_plan "prescaled" reports what the last planned sweeps ran. */
int deff_set_tuning(deff_ctx *ctx, const char *key, int value);
/* what the last launch plan of the temporally blocked kernel chose: "tb_T", "tb_LY" (rows per chunk),
 * "tb_strips", "tb_chunks_per_image", "tb_blocks" (workgroups launched), "tb_impl", "tb_R", "tb_resident" (1: the
 * passes of a batch run as one resident launch; workgroup tiles only), "tb_chain" (1: the streaming kernel chains its passes), "tb_chunk_min" / "tb_chunk_max" (dealt tiles: rows of the shortest and of the tallest chunk), "tb_fallbacks" (resident intervals that gave up and were redone with
 * one launch per pass); 0 before any sweep.  Of the last deff_solve_cg (0 before one): "cg_kr" (rows per work item),
 * "cg_strips" (strips of 128 columns), "cg_items" (work items per image), "cg_restarts" (true-residual rounds that
 * sent an image back into the iteration), "cg_impl" (1 = streaming kernels, 2 = on chip, 3 = on the coefficient planes,
 * 4 = on chip on the coefficient planes: tuning key "cg_onchip_planes") and
 * "cg_fold" (the fold the call ran: 0, 1 or 2, see the tuning key); of the last
 * deff_solve_cg_stream, which also sets the "cg_" keys: "cgs_intervals", "cgs_launches", "cgs_waits" (see there).  Of the
 * last deff_residual / deff_residual_slot / deff_residual_D that launched (0 before one; a refused call leaves them alone):
 * "res_kt" (tiles of 8 rows per run as used: after the planner, the tuning key and the clip to the image's tile rows;
 * 0 after deff_residual_D, which has no runs) and "res_items" (partial sums added per image by the final reduction:
 * strips of 128 columns x ceil(tile rows / res_kt), or for deff_residual_D rows x segments of 256 columns).  Of the last
 * deff_sensitivity / deff_sensitivity_D that launched: "sens_kt" and "sens_items", with the same meaning; of the last
 * deff_field_vjp_D that launched: "vjp_kt" and "vjp_items", of the last deff_tangent_rhs_D: "tan_kt" and "tan_items", and of
 * the last deff_sensitivity_hvp_D: "hvp_kt" and "hvp_items", of the last deff_field_vjp_hvp_D: "fhvp_kt" and "fhvp_items",
 * of the last deff_flux_field / deff_flux_field_D: "flux_kt" and "flux_items" (work items per image),
 * likewise.  Of the flood fill
 * on the device (deff_assemble_3phase_native): "fill_impl" (form of the last fill: 1 = one workgroup per image, 2 = row tiles),
 * "fill_launches" (kernel launches of the last fill), "fill_rounds" (most rounds one workgroup of it took), "fill_runs" (fills
 * computed since the context was created: a continuation stage on the same image computes none), "fill_fallbacks" (images
 * handed to the host fill since then) and "native3_rows" (452 while the system is the native 3-phase one, else 0).  Of the
 * row dictionary: "dict_outcome" (how the harvest of the current explicit system ended: 0 = none tried since the system was
 * set, 1 = harvested, 2 = more distinct rows than the table seats -- 511 beside the zero row, the identity row of an odd
 * width's pad column being one of them --, 3 = the hash table of 16 384 slots overflowed, 4 = the verification pass found a
 * mismatch), "dict_rows" (rows harvested, the zero row not counted; 0 unless the outcome is 1) and "lut_rows" (rows of the
 * current matrix-free table, harvested or a-priori, the zero row counted; 0 without one) */
int deff_get_plan(deff_ctx *ctx, const char *key, int *value);

/* ---- image -> phases: replaces the mask->D loops cuh:1988-2000 (2-phase),
 *      cuh:1518-1529 (3-phase) and the synthetic generator of SURVEY.md 8d */
int deff_set_image(deff_ctx *ctx, const uint8_t *pix, int W, int H, int ampX, int ampY);
int deff_synth_image(deff_ctx *ctx, uint64_t seed, uint64_t img);   /* generated on the device; a stack holds images img, img+1, ... */
int deff_get_image(deff_ctx *ctx, uint8_t *pix);                    /* W*H bytes back */

/* grayscale JPEG file -> bytes: replaces readImage cuh:327-345 (stbi_load(..., 1)); decodes to the
 * same bytes as stb_image v2.26 for one-component files, Huffman-coded baseline, extended sequential
 * and progressive (images up to 2^28 pixels; PNG / BMP get a message); *pix is malloc'ed, release it
 * with deff_free(); host code, needs no context */
int deff_load_jpeg_gray(const char *path, uint8_t **pix, int *W, int *H, int *nChannels);
void deff_free(void *p);

/* ---- assembly: replaces DiscretizeMatrix2D cuh:815-902 (+ WeightedHarmonicMean cuh:347-360) */
/* native 2-phase path: image already on the device, coefficients never leave it */
int deff_assemble_2phase(deff_ctx *ctx, double Ds, double Df, double CL, double CR);
/* drop-in path: caller supplies the per-cell diffusivity D[n] (host); optional
 * Grid[n] selects DiscretizeMatrix2D_ImpSolid cuh:715-812 semantics (NULL = plain) */
int deff_assemble_from_D(deff_ctx *ctx, const double *D, const unsigned int *Grid,
                         double CL, double CR);
/* 3-phase path (SingleSim3Phase cuh:1509-1586): D from pixels (> 200 solid, < 50 gas, else
 * fluid, cuh:1518-1529) on the device + DiscretizeMatrix2D_ImpSolid with Grid (NULL = plain) */
int deff_assemble_3phase(deff_ctx *ctx, double Ds, double Df, double Dg, const unsigned int *Grid,
                         double CL, double CR);
/* FloodFill cuh:557-713 on the host, linear time: Grid[n] (1 = solid) gets 2 where the pore
 * space is not connected to the left wall; *path_flag = PathFlag.  Needs no context. */
int deff_flood_fill(unsigned int *Grid, int nx, int ny, int *path_flag);
/* native 3-phase path: the 3-phase system with the flood-filled Grid (what deff_flood_fill on `pixel > 200` followed by
 * deff_assemble_3phase gives, the same doubles) without leaving the device.  The connectivity of the pore space is computed
 * from the context's pixels by a flood fill on bitmaps (per image of a stack: 4-connected, periodic between the image's
 * first and last row, seeded from column 0, the reference's right-column quirk cuh:601 included); every cell gets a 16-bit
 * row code and the row table is enumerated a priori (452 rows: identity for Grid 1 / 2, else the cell's phase and its
 * existing neighbours' pixel classes per position class).  The fill is computed when the context has none for its current
 * image (deff_set_image / deff_synth_image invalidate it); a further call on the same image -- a continuation stage with
 * another Dg -- rebuilds the table and the wall diffusivities only.  Explicit planes are built on demand (deff_get_system,
 * DEFF_KERNEL_EXPLICIT / _SCALAR, "cg_planes").  Everything downstream runs as on a harvested 3-phase dictionary and gives
 * the same bits.  An image the device fill cannot finish within its launch budget is filled on the host (deff_get_plan
 * "fill_fallbacks"), which is not an error.  Row-slab contexts: DEFF_EINVAL; no image: DEFF_ESTATE; a refusal leaves the
 * field and the previous system as they were.  Tuning keys "fill_impl", "fill_tile_rows". */
int deff_assemble_3phase_native(deff_ctx *ctx, double Ds, double Df, double Dg, double CL, double CR);
/* the device fill of the current image in FloodFill's encoding (0 reached, 1 solid, 2 not reached) and the PathFlag of
 * every image (the flags are on the host already: with Grid NULL nothing is copied); DEFF_ESTATE before a fill exists */
int deff_get_grid(deff_ctx *ctx, unsigned int *Grid /* nimg*ny*nx, may be NULL */, int *path_flag /* [nimg], may be NULL */);
/* host-assembled system as the reference passes it to JacobiGPU (cuh:1163):
 * A[n*5] AoS, b[n], D[n] (only its first and last column are read, cuh:1256-1257) */
int deff_set_system(deff_ctx *ctx, const double *A, const double *b, const double *D,
                    double CL, double CR);
/* assembled coefficients back in the reference's AoS layout (parity tests, drop-in) */
int deff_get_system(deff_ctx *ctx, double *A, double *b);
/* the matrix-free form as the matrix-free kernels see it, harvested and a-priori tables alike: rows[R * 6] = a0, aW, aE, aS,
 * aN, b of the table's R rows (R = deff_get_plan "lut_rows"; row 0 is the zero row), codes[nimg*ny * pitch] = every cell's
 * code (8 x its row index) with pitch = nx rounded up to even -- the pad column of an odd mesh width included.  Either
 * pointer may be NULL.  Read-only.  DEFF_ESTATE when the system has no matrix-free form.
 * A harvested table is ordered by population, most cells first; rows of equal population by the bit patterns of their six
 * doubles, compared as unsigned 64-bit integers in the order above.  The codes are therefore a function of the system. */
int deff_get_dictionary(deff_ctx *ctx, double *rows, uint16_t *codes);

/* ---- field ------------------------------------------------------------- */
int deff_init_linear(deff_ctx *ctx, double CL, double CR);          /* cuh:1955-1959 */
int deff_set_field(deff_ctx *ctx, const double *x);                 /* H2D of the guess, cuh:1203 */
int deff_get_field(deff_ctx *ctx, double *x);                       /* final D2H, cuh:1300 */

/* ---- solve: replaces JacobiGPU cuh:1163-1314 / JacobiGPUPreCond cuh:1024-1160
 * and the kernels updateX_SOR cuh:69-92 (omega = 2/3) / updateX_V1 cuh:96-118 (omega = 1).
 * Stopping rule exactly as cuh:1232-1290: check when iter % check_every == 0
 * (including iter 0), deffOld seeded with 5, stop when |change| <= tol or
 * iter == max_iter.  MFL/MFR (ny doubles each, may be NULL) receive the wall
 * fluxes of the last check (cuh:1256-1257). */
int deff_solve(deff_ctx *ctx, double omega, double tol, int64_t max_iter, int64_t check_every,
               deff_result *out, double *MFL, double *MFR);
/* same loop for a batch context: out[nimg]; each image stops by its own rule (its sweeps
 * end, its field is frozen) while the others continue; MFL/MFR hold nimg*ny values */
int deff_solve_batch(deff_ctx *ctx, double omega, double tol, int64_t max_iter, int64_t check_every,
                     deff_result *out, double *MFL, double *MFR);
/* Preconditioned conjugate gradients to a residual tolerance (opt-in; NOT the reference's algorithm -- the reference
 * has only the weighted Jacobi loop above).  Jacobi-preconditioned CG in FP64 on the matrix-free form converges to the
 * same discrete fixed point (the same A, b and wall-flux Deff) in far fewer iterations.  The current field is the
 * initial guess (deff_init_linear / deff_set_field); the solution is written into it, so deff_get_field, deff_flux,
 * deff_residual and deff_device_field see it afterwards.  Plain and stack contexts (out[nimg], MFL/MFR nimg*ny values,
 * may be NULL).  An image stops when ||r||_2 <= rtol * ||b||_2 (on the device, whatever check_every: the host looks at
 * the images' flags every check_every iterations only; the results do not depend on it); the residual is then
 * recomputed from x and the iteration restarted if it misses rtol.  Decoupled rows (four zero links and b = 0: cells
 * outside the mesh, ImpSolid / FloodFill rows, a phase with D = 0) get x = 0 -- where the Jacobi loop of a 2-phase
 * system with Ds = 0 gives NaN, CG gives a finite field.  A right-hand side of zero (||b|| = 0): a field with A x = 0
 * returns at once with rel_residual 0, converged; any other field has rel_residual = inf, iterates to max_iter (the
 * stop test ||r|| <= rtol * 0 never holds) and returns not converged with a finite field.  DEFF_EINVAL: row-slab contexts (one image
 * over row slabs: deff_slab_group_solve_cg / deff_slab_rank_solve_cg below), systems without a row
 * dictionary or explicit-only ones (a wall link into the neighbouring row), and systems that are not symmetric (a link
 * between two active cells that differs from its partner, an active row with A0 <= 0); nothing is changed then.
 * Tuning key "cg_onchip" (0 default: the streaming kernels, four launches per iteration): 1 = when an image of the context
 * has at most 16 384 cells (row pitch x ny, the pitch being nx rounded up to even: 128 x 128, 8192 x 2, 2 x 8192 ...), every
 * image is iterated by one workgroup that keeps x, r, p and the codes in one compute unit's registers and LDS; check_every
 * iterations are then ONE launch, and a stack's images run side by side, one per compute unit.  Larger images keep the
 * streaming kernels.  Same recurrence, stop rules, true-residual rounds and results as above (the dot products are summed
 * in another fixed order, so the bits differ from the streaming form's; they do not depend on check_every or on the
 * stack an image is in).  deff_get_plan "cg_impl" tells which form the last call ran: 1 = streaming, 2 = on chip.
 * Tuning key "cg_planes" (0 default: as above, a system without a row dictionary is refused): the iteration reads the matrix
 * from the explicit coefficient planes (a0, aW, aE, aS, aN, b per cell) instead of the row codes and the dictionary -- for a
 * diffusivity that varies cell by cell (deff_assemble_from_D), a caller's own assembly (deff_set_system), more distinct rows
 * than a dictionary holds, or a context with the tuning key "dict" 0.  1 = when the system has no dictionary after one has
 * been looked for; a system that has one runs as above ("cg_onchip" included).  2 = for every system: a native system's
 * planes are built from its image, the dictionary is neither looked for nor touched and "cg_onchip" has no effect; a system
 * that has a dictionary gives the bits of the table form (same work items, expressions and summation order).  Everything
 * said above holds for this form -- guess and solution in the field, the stop on the device, results independent of
 * check_every, the true-residual rounds, rel_residual from the field, decoupled rows at x = 0, an image of a stack solved
 * as alone -- and the system's admissibility is checked on the device before the field is touched (same refusals).
 * deff_get_plan "cg_impl" = 3; "cg_kr", "cg_strips", "cg_items", "cg_restarts" keep their meaning.  The planes, the row
 * dictionary and every plan of the Jacobi path are left as they are.  Still refused whatever the key: explicit-only systems
 * (a wall link into the neighbouring row) and row-slab contexts; the key has no effect on deff_slab_*_solve_cg (a slab's
 * system needs a dictionary) nor on deff_solve_cg_stream (a native 2-phase system always has one).
 * Tuning key "cg_onchip_planes" (0 default: nothing changes anywhere; values above 1 are DEFF_EINVAL): 1 = a solve that takes
 * the plane form -- this call when the system has no dictionary under "cg_planes" 1 or under "cg_planes" 2, and
 * deff_solve_adjoint, deff_solve_tangent and deff_solve_adjoint_tangent always -- iterates every image by one workgroup on one
 * compute unit, as "cg_onchip" does for the table form, when an image has at most 16 384 cells (row pitch x ny, the same rule).
 * r and A p stay in registers and p in LDS; a pair's matrix row and 1 / A0 are read from the coefficient planes and the
 * field is read and written in place in every iteration (72 B per cell through L2 / Infinity Cache).  The start, the admissibility check, the flag reads every check_every
 * iterations, the true-residual rounds and the fluxes are the streaming plane form's; the mapping and the order of the sums
 * are the table on-chip form's, so a system that has a dictionary gives the bits of "cg_onchip" 1, and any system bits that
 * do not depend on check_every or on the stack an image is in.  deff_get_plan "cg_impl" = 4 and "cg_fold" = 0 after such a
 * call.  Larger images, and every call under 0, run exactly as without the key.  Independent of "cg_onchip", which keeps its
 * meaning for systems that run on the row table.  No effect on row slabs nor on deff_solve_cg_stream.
 * Tuning key "cg_fold" (0 default: four launches per iteration -- two that stream over the field, two that run one
 * workgroup per image to add its partial sums and set alpha / beta and the stop flags): 1 = two launches per iteration.
 * Every work item counts itself in when its partial sum is stored, and the last workgroup to arrive for an image adds the
 * image's partial sums, in the order the separate launch adds them, and does that launch's step; no workgroup waits for
 * another.  2 = as 1, and the table form's direction kernel keeps the loads of a row ahead in flight (on the coefficient
 * planes 2 means 1: that kernel loads ahead already).  Values above 2 are DEFF_EINVAL.  The results are those of 0 bit for
 * bit -- fields, iteration counts, rel_residual, converged, deff_raw, the wall fluxes, "cg_kr", "cg_strips", "cg_items",
 * "cg_restarts" -- for every system, stack and check_every.  The key applies to the streaming kernels of deff_solve_cg
 * ("cg_impl" 1 and 3, plain and stack contexts) and of deff_solve_cg_stream, whose "cgs_launches" drops by two per enqueued
 * iteration; it has no effect on the on-chip form ("cg_impl" 2) nor on row slabs (deff_slab_*_solve_cg: their gathers are
 * a reduction of their own).  The start of a call and the true-residual rounds keep their own launches.
 * deff_get_plan "cg_fold" tells what the last CG call ran: 0, 1 or 2; 0 when it ran on chip, and before any call. */
typedef struct deff_cg_result {
    int64_t iters;         /* CG iterations of this image */
    double  rel_residual;  /* ||b - A x||_2 / ||b||_2 of the returned field, recomputed from x */
    double  deff_raw;      /* Deff of the returned field (cuh:1252-1263 expressions), not / Df */
    double  loop_ms;       /* hipEvent time of the CG loop (shared by the images of a stack) */
    int     converged;     /* rel_residual <= rtol */
} deff_cg_result;
int deff_solve_cg(deff_ctx *ctx, double rtol, int64_t max_iter, int64_t check_every,
                  deff_cg_result *out /* [nimg] */, double *MFL, double *MFR);
/* streaming batch (dataset generation): the nimg slots of a batch context are kept full -- when a
 * slot's image stops (its own rule), its result is reported and the slot is refilled with the next
 * image, which enters one sweep before a check of the running ones so that every image keeps the
 * reference's schedule (checks after its own sweeps 1, C+1, 2C+1, ...).  2-phase native system.
 *   next(user, slot, pix, &image_id) fills W*H bytes: 1 = image provided, 0 = no more, <0 = error
 *   done(user, image_id, slot, result): called once per image; deff_get_slot_field(ctx, slot, x)
 *   may be called from inside it to fetch the image's final field */
typedef int (*deff_next_image_fn)(void *user, int slot, uint8_t *pix, int64_t *image_id);
typedef void (*deff_image_done_fn)(void *user, int64_t image_id, int slot, const deff_result *res);
/* After DEFF_OK the context is an ordinary stack context: slot k holds the last image that ran in it (the slot `done` reported
 * for it), the 2-phase system of this call's Ds, Df, CL, CR, and that image's FINAL field, whatever buffer the image was
 * frozen in while other slots kept sweeping.  A slot that never received an image (fewer images than slots) holds pixels
 * of 0, zero rows, zero wall diffusivities and a zero field (Deff 0): it reads 0 and its Deff and residual are finite.  That
 * is a place holder, not the system of an image: what later sweeps make of such a slot depends on the kernel (the kernels
 * that read row codes keep it at 0, the ones that read coefficient planes rebuild them from the pixels of 0) and is
 * unspecified until deff_set_image and an assembly give the slot an image.  Every later call behaves as on a stack assembled
 * that way by hand: deff_get_field, deff_get_slot_field, deff_flux, deff_residual, deff_residual_slot, deff_sweeps,
 * deff_solve_batch, deff_solve_cg, deff_device_field, a new image and re-assembly.  The same holds when no sweep ran at all
 * (max_iter <= 0, or tol >= 100, the change the stopping rule is seeded with): the fields are then the linear guesses. */
int deff_solve_stream(deff_ctx *ctx, int W, int H, int ampX, int ampY, double Ds, double Df, double CL,
                      double CR, double omega, double tol, int64_t max_iter, int64_t check_every,
                      deff_next_image_fn next, deff_image_done_fn done, void *user);
int deff_get_slot_field(deff_ctx *ctx, int slot, double *x /* nx*ny */);
/* Conjugate gradients through refilled slots (dataset generation with converged fields): the slot life cycle of
 * deff_solve_stream around the iteration of deff_solve_cg.  Batch contexts, native 2-phase system; `next` as above.  Every image
 * is solved exactly as a one-image deff_solve_cg call would solve it from the linear guess (deff_init_linear): the same
 * recurrence, the same stop per image (||r|| <= rtol ||b||, max_iter, breakdown), the same true-residual round at its end with
 * up to 8 restart rounds per image; rel_residual is recomputed from the field, converged derived from it, deff_raw is the
 * slot's deff_flux value, loop_ms the hipEvent time from the start of the call to the check that retired the image.  The
 * results (bits) do not depend on check_every, on the number of slots or on the slot and neighbours an image had.  With the
 * tuning key "cg_onchip" 1, images of at most 16 384 cells iterate on one compute unit each; everything else runs the
 * streaming kernels (deff_get_plan "cg_impl": 2 / 1).
 *   The device does not wait for the host: the iterations of the next check interval (check_every of them) are enqueued before
 * the host reads what the last one left; a slot found stopped is frozen until its true-residual round, flux, `done`, the next
 * image's upload and entry have run behind that interval, and rejoins with the interval after it.  Launches and host waits per
 * interval do not grow with the number of slots that retire or enter.  (An interval in which a slot retires still has a turn
 * of the host that the device waits for: the wait for the round comes behind the interval already enqueued, and `done`, `next`
 * and the upload run before the interval after it is enqueued.)  deff_get_plan, of the last stream: "cgs_intervals",
 * "cgs_launches" = kernel launches enqueued, "cgs_waits" = host waits on the device.
 *   done(user, image_id, slot, result): once per image; deff_get_slot_field and deff_residual_slot work for `slot` inside it.
 *   DEFF_EINVAL before `next` is ever called: NULL callbacks, rtol negative or not finite, max_iter < 0, check_every < 1, a
 * row-slab context, an image that does not match the mesh, a table that is not admissible (an active row without a finite
 * A0 > 0, e.g. Df < 0 or not finite; the rule is deff_solve_cg's, so Df = 0 or Ds = 0 is admitted: that phase's rows are
 * decoupled and its cells get x = 0).  Such a refusal changes nothing: image, fill, system (a native 3-phase one included),
 * field and plans are what they were.  A `next` that returns < 0: DEFF_EINVAL.  The symmetry of an entering slot's system is checked on the
 * device and reported (DEFF_EINVAL) with the next look at the slots.
 *   After DEFF_OK the context is an ordinary stack context, as after deff_solve_stream: slot k holds the last image that ran in
 * it, its system and its final field; slots that never received an image hold the zero place holder described above. */
typedef void (*deff_cg_image_done_fn)(void *user, int64_t image_id, int slot, const deff_cg_result *res);
int deff_solve_cg_stream(deff_ctx *ctx, int W, int H, int ampX, int ampY, double Ds, double Df, double CL, double CR,
                         double rtol, int64_t max_iter, int64_t check_every,
                         deff_next_image_fn next, deff_cg_image_done_fn done, void *user);
/* optional observer called on the host after every convergence check with
 * (iter of the checked sweep, Deff, signed change): what the reference prints under
 * Verbose (cuh:1267-1271).  NULL removes it. */
typedef void (*deff_progress_fn)(int64_t iter, double deff_raw, double change, void *user);
int deff_set_progress(deff_ctx *ctx, deff_progress_fn fn, void *user);
/* building blocks, also used by bench.py: n sweeps without a check (ms = hipEvent
 * time on the context's stream), and one flux / Deff evaluation (cuh:1252-1263) */
int deff_sweeps(deff_ctx *ctx, int64_t n, double omega, float *ms);
int deff_flux(deff_ctx *ctx, double *deff_raw /* [nimg] */, double *MFL, double *MFR);
/* Residual() cuh:451-494 of the current field: r[k] = mean over the cells of image k of |qW - qE + qN - qS| (the reference
 * defines it and leaves its two call sites, cuh:1121 and cuh:1266, commented out).  Every cell's term is the reference's
 * arithmetic; the sum is a wavefront-level reduction in a fixed order (deterministic; ~1e-16 relative from the reference's
 * serial row-major order).  deff_residual: systems assembled from the image (deff_assemble_2phase / _3phase; no D plane is
 * read: 9 B per cell); deff_residual_D: any diffusivity plane D[ny*nx] (host), the reference's own call shape.  Both may be
 * called from a deff_set_progress() callback.  *ms (may be NULL) = device time of the reduction.  Not for slab contexts. */
int deff_residual(deff_ctx *ctx, double *r /* [nimg] */, float *ms);
/* ... of ONE image of a stack, wherever its newest field lives: callable from the deff_image_done_fn callback of a stream */
int deff_residual_slot(deff_ctx *ctx, int slot, double *r);
int deff_residual_D(deff_ctx *ctx, const double *D, double CL, double CR, double *r /* [nimg] */, float *ms);
/* The Deff gradient of the current field, meaningful for a CONVERGED one (deff_solve_cg): g[p] = d deff_raw / d D[p] for every
 * cell, in one pass over the field and the diffusivities -- the problem is self-adjoint, no second solve.  With dx, dy of
 * deff_mesh, wx = dy / dx for W / E faces, wy = dx / dy for N / S faces (the assembly's weights), each face of cell p adds
 *   interior, to q:  s = Dp + Dq;  t = (s == 0) ? 0 : Dq / s;  e = xp - xq;  c = (2.0 * (t * t)) * (w * (e * e))
 *   left / right wall:  e = xp - CL (CR);  c = (dy / (dx / 2.0)) * (e * e);      no face (first / last row):  c = +0.0
 *   g[p] = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL)),  and g[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/sensitivity_model.py states them in numpy).  euler[k] = sum over image k of D[p] * g[p],
 * which equals deff_raw for the exact solution (Deff is homogeneous of degree 1 in D): a wave-level reduction in a fixed order
 * (csrc/kernels_sens.hpp), the same bits on every call.  g (nimg*ny*nx, true width) and euler ([nimg]) may each be NULL;
 * *ms (may be NULL) = device time of the pass, on an event pair of its own.
 *   deff_sensitivity_D: D[nimg*ny*nx] on the host, as deff_assemble_from_D takes it, with the wall values.
 *   deff_sensitivity: D from the context's image system -- deff_assemble_2phase, or deff_assemble_3phase with Grid == NULL --,
 *     filled on the device from the stored phase diffusivities; CL, CR are the system's.  A system assembled with a Grid
 *     (ImpSolid rows, deff_assemble_3phase_native) is DEFF_EINVAL; deff_set_system, deff_assemble_from_D or no system: DEFF_ESTATE.
 * Plain and stack contexts; row slabs and CR == CL are DEFF_EINVAL.  Pending work is settled first and every image's newest
 * field is read; nothing else changes (field, system, plans, tuning, the solvers' timing), and a refused call leaves the
 * previous map alone.  Negative or non-finite D: unspecified values, never a fault.
 * Tuning "sens_kt": tiles of 8 rows one wave streams through (0 = the planner's choice, clipped to the image);
 * deff_get_plan "sens_kt" / "sens_items": what the last call used, and the partial sums added per image
 * (strips of 128 columns x ceil(tile rows / sens_kt)).
 * deff_device_sensitivity: the device buffer of the last map (row pitch as deff_device_field), valid until the next
 * sensitivity call, assembly or deff_destroy; DEFF_ESTATE before one exists. */
int deff_sensitivity_D(deff_ctx *ctx, const double *D, double CL, double CR,
                       double *g /* nimg*ny*nx, may be NULL */, double *euler /* [nimg], may be NULL */, float *ms);
int deff_sensitivity(deff_ctx *ctx, double *g, double *euler, float *ms);
int deff_device_sensitivity(deff_ctx *ctx, void **d_g, size_t *row_pitch_bytes);
/* The flux field of the current field: the flux through every face and the total flux through every vertical section, in one
 * pass over the field and the diffusivities (nothing like it in the reference, which evaluates the two wall columns only,
 * cuh:1256-1257).  With dx, dy of deff_mesh, whm(w1, w2, x1, x2) = (w1 + w2) / (w1 / x1 + w2 / x2) (cuh:347-360), row 0 the
 * top row, e the east and s the south (row + 1) neighbour of cell p:
 *   interior E face:  ke = whm(dx / 2, dx / 2, Dp, De);  fx[p] = ((ke * dy) / dx) * (xe - xp)
 *   right wall (the last column):  fx[p] = ((Dp * dy) / (dx / 2)) * (CR - xp)
 *   left wall (column 0):  left[row] = ((Dp * dy) / (dx / 2)) * (xp - CL)
 *   interior S face:  ks = whm(dy / 2, dy / 2, Ds, Dp);  fy[p] = ((ks * dx) / dy) * (xs - xp)
 *   last row of an image:  fy[p] = +0.0 (nothing crosses between the images of a stack)
 * These doubles, in this order (tests/flux_model.py states them in numpy; the library is built without contraction): the
 * conductances of the assembly (DiscretizeMatrix2D) in its operation order.  With fxW[p] the east flux of the west neighbour
 * (or left) and fyN[p] the south flux of the north neighbour (or 0), fxW - fx + fyN - fy at cell p equals (A x - b)[p] up to
 * rounding.  Sign: the reference's Residual(), "higher index minus lower"; the physical flux is the negative.  Weights:
 * Residual() (cuh:479-485) weights vertical faces with dy / dx, the assembly with dx / dy; this pass follows the ASSEMBLY, so
 * the identity holds on meshes whose cells are not square.  D == 0 needs no special case (whm returns 0, the flux is 0).
 * sections: per image W + 1 sums, W the mesh width: Q[0] = sum over the rows of left, Q[j] = sum over the rows of
 *   fx[row, j - 1], Q[W] the right wall; (Q[0] + Q[W]) / (2 (CR - CL)) is deff_raw up to rounding, and with no-flux top and
 *   bottom all W + 1 are the same number for a converged field: their spread says how far Deff depends on where it is measured.
 *   Order of a sum, fixed: the rows of an image are cut into runs of 8 * "flux_kt" rows; within a run a column's terms are
 *   added top to bottom, starting from the first; the runs are added in order, starting from the first.  The same bits on
 *   every call.
 * fx, fy (nimg*ny*nx, true width), left (nimg*ny) and sections (nimg*(nx+1)) may each be NULL; *ms (may be NULL) = device
 * time of the pass, on an event pair of its own.
 *   deff_flux_field_D: D[nimg*ny*nx] on the host, as deff_sensitivity_D takes it.  CR == CL is allowed (nothing is divided by it).
 *   deff_flux_field: D from the context's image system -- deff_assemble_2phase, or deff_assemble_3phase with Grid == NULL --,
 *     filled on the device from the stored phase diffusivities; CL, CR are the system's.  A system assembled with a Grid
 *     (ImpSolid rows, deff_assemble_3phase_native) is DEFF_EINVAL; no image system: DEFF_ESTATE.  A new image
 *     (deff_set_image, deff_synth_image) leaves none until the next assembly, here and for deff_sensitivity and deff_residual.
 * Plain and stack contexts; row slabs, NULL ctx and NULL D: DEFF_EINVAL; no field: DEFF_ESTATE.  Pending work is settled first
 * and every image's newest field is read.  A successful call writes only its own buffers and the upload scratch -- not the
 * field, the system, the plans, the other passes' maps or the solvers' events --, and a refused call changes nothing.
 * Negative or non-finite D: unspecified values, never a fault.
 * Tuning "flux_kt": tiles of 8 rows one wave streams through (0 = the planner's choice, clipped to the image);
 * deff_get_plan "flux_kt" / "flux_items": what the last call used, and its work items per image
 * (strips of 128 columns x ceil(tile rows / flux_kt)).
 * deff_device_flux_field: the device buffers of the last maps (row pitch as deff_device_field, the pad column of an odd width
 * holds +0.0), valid until the next flux-field call or deff_destroy; DEFF_ESTATE before the first call. */
int deff_flux_field_D(deff_ctx *ctx, const double *D, double CL, double CR,
                      double *fx, double *fy /* nimg*ny*nx, may be NULL */, double *left /* nimg*ny, may be NULL */,
                      double *sections /* nimg*(nx+1), may be NULL */, float *ms);
int deff_flux_field(deff_ctx *ctx, double *fx, double *fy, double *left, double *sections, float *ms);
int deff_device_flux_field(deff_ctx *ctx, void **d_fx, void **d_fy, size_t *row_pitch_bytes);
/* ---- field adjoint: dL/dD for ANY loss L(x) on the concentration field, one adjoint solve and one pass (nothing like it in
 * the reference).  The system is A(D) x = b(D) with A symmetric, so for w = dL/dx the adjoint system is the same matrix:
 * A lambda = w with homogeneous walls, and dL/dD[p] = -lambda^T (dA/dD[p] x - db/dD[p]), a face-wise pass over (x, lambda, D).
 *
 * deff_solve_adjoint: A lambda = w on the context's CURRENT matrix; lambda goes into a buffer of the context's own.
 *   Reads: the system (its coefficient planes; a native 2- / 3-phase system's are built from its image first, as under the
 *   tuning key "cg_planes" 2) and w[nimg*ny*nx] on the host, true width.  Needs neither a field nor wall diffusivities.
 *   The iteration is deff_solve_cg's on the coefficient planes, whatever "cg_planes" and "cg_onchip" are set to ("cg_fold"
 *   applies as it does to that form; under "cg_onchip_planes" 1 images of at most 16 384 cells iterate on one compute unit
 *   each, "cg_impl" 4, here and in deff_solve_tangent and deff_solve_adjoint_tangent): the same work items, recurrence and summation order, the same stop on the device
 *   (||r|| <= rtol ||w'||), the same true-residual rounds and restart limit, results independent of check_every.  The guess
 *   is always lambda = 0.  Which cells are decoupled is decided by the FORWARD system (four zero links and forward b == 0):
 *   there w is ignored (w' = 0) and lambda = 0; everywhere else w' = w.  An image with ||w'|| = 0 returns at once: iters 0,
 *   rel_residual 0, converged 1, lambda = 0.  out[k].rel_residual = ||w' - A lambda|| / ||w'|| recomputed from lambda,
 *   out[k].deff_raw is 0.0 (lambda has no flux), loop_ms as in deff_solve_cg.  Non-finite w: unspecified values, never a fault.
 *   Writes: lambda, w', the CG work vectors, the upload scratch and the "cg_*" plan keys ("cg_impl" 3).  Left as they are: the
 *   field and which buffer holds it, b and every other coefficient plane, the row dictionary, the Jacobi plans and tuning,
 *   the sensitivity map and the events the solve loops time themselves with.
 *   Refusals, each changing nothing: NULL ctx / w / out, rtol negative or not finite, max_iter < 0, check_every < 1, a row-slab
 *   context, an explicit-only system (a wall link into the neighbouring row), a system that is not admissible or not symmetric
 *   (deff_solve_cg's verdict on the forward planes): DEFF_EINVAL; no system: DEFF_ESTATE.
 * The adjoint field's lifetime: deff_solve_adjoint and deff_set_adjoint make it valid; every call that replaces the system or
 *   the image (the deff_assemble_* calls, deff_set_system, deff_set_image, deff_synth_image, deff_solve_stream,
 *   deff_solve_cg_stream) invalidates it.  While it is invalid deff_get_adjoint, deff_device_adjoint and deff_field_vjp_D
 *   return DEFF_ESTATE.
 * deff_set_adjoint: lam[nimg*ny*nx] (host, true width) becomes the adjoint field -- a caller's own lambda.  deff_get_adjoint:
 *   the adjoint field back.  deff_device_adjoint: its device buffer, row pitch as deff_device_field (the pad column of an odd
 *   width holds 0); valid until the context is destroyed, its contents until the next deff_solve_adjoint / deff_set_adjoint.
 *   NULL arguments and row-slab contexts: DEFF_EINVAL.
 *
 * deff_field_vjp_D: g[p] = dL/dD[p] from the current field x, the current lambda and D, in one pass.  With dx, dy of deff_mesh,
 * wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), x and l (lambda) of cell p and of its neighbour q:
 *   interior face of p towards q (weight w = wx for W / E, wy for N / S):
 *       s = Dp + Dq;  t = (s == 0) ? 0 : Dq / s;  e = xp - xq;  f = lp - lq;  c = (2.0 * (t * t)) * (w * (e * f))
 *   left / right wall:  e = xp - CL (CR);  f = lp;  c = ww * (e * f)          no face (first / last row of an image):  c = +0.0
 *   g[p] = -(((cW + cE) + cN) + cS),   and g[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/field_vjp_model.py states them in numpy; the library is built without contraction).
 * euler[k] = sum over image k of D[p] * g[p]: A and b are homogeneous of degree 1 in D, so x is of degree 0 and the sum is
 * -lambda^T (A x - b) = 0 for a converged x, whatever lambda is -- a check that needs no reference.  It is a wave-level
 * reduction in a fixed order (csrc/kernels_vjp.hpp), the same bits on every call.  g (nimg*ny*nx, true width) and euler
 * ([nimg]) may each be NULL; *ms (may be NULL) = device time of the pass, on an event pair of its own.
 *   D[nimg*ny*nx] on the host, as deff_sensitivity_D takes it.  CR == CL is allowed (nothing is divided by it).
 *   Plain and stack contexts; row slabs: DEFF_EINVAL; NULL ctx or D: DEFF_EINVAL; no field, or no valid lambda: DEFF_ESTATE.
 *   Pending work is settled first and every image's newest field is read.  The call writes only its own map, its partial sums
 *   and the upload scratch; a refused call leaves the previous map alone.  Negative or non-finite D: unspecified values,
 *   never a fault.
 * Tuning "vjp_kt": tiles of 8 rows one wave streams through (0 = the planner's choice -- the gradient pass's planner --, values
 * above the image's tile rows are clipped); deff_get_plan "vjp_kt" / "vjp_items": what the last call used, and the partial sums
 * added per image (strips of 128 columns x ceil(tile rows / vjp_kt)).
 * deff_device_field_vjp: the device buffer of the last map (row pitch as deff_device_field), valid until the next
 * deff_field_vjp_D or deff_destroy; DEFF_ESTATE before one exists. */
int deff_solve_adjoint(deff_ctx *ctx, const double *w /* nimg*ny*nx, host, true width */, double rtol, int64_t max_iter,
                       int64_t check_every, deff_cg_result *out /* [nimg] */);
int deff_set_adjoint(deff_ctx *ctx, const double *lam);
int deff_get_adjoint(deff_ctx *ctx, double *lam);
int deff_device_adjoint(deff_ctx *ctx, void **d_lam, size_t *row_pitch_bytes);
int deff_field_vjp_D(deff_ctx *ctx, const double *D, double CL, double CR,
                     double *g /* nimg*ny*nx, may be NULL */, double *euler /* [nimg], may be NULL */, float *ms);
int deff_device_field_vjp(deff_ctx *ctx, void **d_g, size_t *row_pitch_bytes);
/* ---- field tangent: dx = (dx/dD) dD, the field's derivative along a direction dD of the diffusivity map, one pass and one
 * solve (nothing like it in the reference): the forward-mode counterpart of the field adjoint, J v where that gives J^T w.
 * Differentiating A(D) x = b(D) along dD:  A dx = db - dA x =: r  with homogeneous walls, the same matrix again.
 *
 * deff_tangent_rhs_D: r[p] from the current field x, D and dD, in one pass.  With dx, dy of deff_mesh, wx = dy / dx,
 * wy = dx / dy, ww = dy / (dx / 2.0), d[p] = (D[p] == 0) ? 0 : dD[p], x and d of cell p and of its neighbour q:
 *   interior face of p towards q (weight w = wx for W / E, wy for N / S):
 *       s = Dp + Dq;  tq = (s == 0) ? 0 : Dq / s;  tp = (s == 0) ? 0 : Dp / s;
 *       h = (2.0 * (tq * tq)) * dp + (2.0 * (tp * tp)) * dq;  e = xp - xq;  c = w * (h * e)
 *   left / right wall:  c = ww * (dp * (xp - CL (CR)))          no face (first / last row of an image):  c = +0.0
 *   r[p] = -(((cW + cE) + cN) + cS),   and r[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/tangent_model.py states them in numpy; the library is built without contraction).  h is
 * the change of the face's harmonic mean; it has the same bits seen from either cell and e changes sign exactly, so a face
 * is evaluated once for both.  norm2[k] = sum over image k of r[p] * r[p], a wave-level reduction in a fixed order
 * (csrc/kernels_facepass.hpp), the same bits on every call.  x is of degree 0 in D, so for dD = D the pass returns the
 * forward residual b - A x and norm2 its squared norm: ~0 for a converged x, a check that needs no reference.  r
 * (nimg*ny*nx, true width) and norm2 ([nimg]) may each be NULL; *ms (may be NULL) = device time of the pass, on an event
 * pair of its own.
 *   D and dD [nimg*ny*nx] on the host, as deff_field_vjp_D takes D.  CR == CL is allowed.
 *   Plain and stack contexts; row slabs: DEFF_EINVAL; NULL ctx, D or dD: DEFF_EINVAL; no field: DEFF_ESTATE.  Needs no system.
 *   Pending work is settled first and every image's newest field is read.  The call writes only its own map, its partial sums
 *   and the upload scratch (which holds both planes: 2 n doubles); a refused call leaves the previous map alone.  Negative or
 *   non-finite D or dD: unspecified values, never a fault.
 * Tuning "tan_kt" and deff_get_plan "tan_kt" / "tan_items": as "vjp_kt" / "vjp_items", the same planner.
 * deff_device_tangent_rhs: the device buffer of the last map (row pitch as deff_device_field, the pad column of an odd width
 *   holds 0), valid until the next deff_tangent_rhs_D or deff_destroy; DEFF_ESTATE before one exists.
 *
 * deff_solve_tangent: A dx = r' on the context's CURRENT matrix, r' = the last deff_tangent_rhs_D's map with the forward
 *   system's decoupled rows zeroed, read on the device (no host round trip); dx goes into a buffer of the context's own.
 *   Everything else is deff_solve_adjoint with w = r, bit for bit: the iteration on the coefficient planes from the guess 0,
 *   "cg_fold", the stop, the true-residual rounds, out[k] (deff_raw 0.0).
 *   Writes: dx, r' (a copy: the map stays as it was), the CG work vectors and the "cg_*" plan keys.  Left as they are: lambda
 *   and its validity, the field, the system, the row dictionary, the Jacobi plans, the sensitivity and field-adjoint maps.
 *   Refusals, each changing nothing: those of deff_solve_adjoint, and DEFF_ESTATE while there is no right-hand side map for
 *   the current system.
 * The tangent's lifetime: deff_solve_tangent and deff_set_tangent (below) make dx valid; every call that invalidates the adjoint field (see there)
 *   invalidates dx and the map's use as a right-hand side -- a new deff_tangent_rhs_D is needed; deff_device_tangent_rhs still
 *   hands the old map out.  While dx is invalid deff_get_tangent and deff_device_tangent return DEFF_ESTATE.
 * deff_get_tangent: dx[nimg*ny*nx] to the host, true width.  deff_device_tangent: its device buffer, row pitch as
 *   deff_device_field; valid until the context is destroyed, its contents until the next deff_solve_tangent.  NULL arguments
 *   and row-slab contexts: DEFF_EINVAL.
 * A Gauss-Newton product J^T (J v): deff_tangent_rhs_D(v), deff_solve_tangent, deff_get_tangent, deff_solve_adjoint(w = dx),
 *   deff_field_vjp_D. */
int deff_tangent_rhs_D(deff_ctx *ctx, const double *D, const double *dD, double CL, double CR,
                       double *r /* nimg*ny*nx, may be NULL */, double *norm2 /* [nimg], may be NULL */, float *ms);
int deff_device_tangent_rhs(deff_ctx *ctx, void **d_r, size_t *row_pitch_bytes);
int deff_solve_tangent(deff_ctx *ctx, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out /* [nimg] */);
int deff_get_tangent(deff_ctx *ctx, double *dx);
int deff_device_tangent(deff_ctx *ctx, void **d_dx, size_t *row_pitch_bytes);
/* ---- Deff Hessian-vector product: hv = H dD, H the Hessian of deff_raw with respect to the diffusivity map, one tangent
 * solve and one pass (nothing like it in the reference): what Newton-CG, trust-region steps and curvature checks on a
 * diffusivity map need.  g(D) = d deff_raw / dD at the converged field is deff_sensitivity_D's map, a function of (x, D); along
 * a direction dD,  H dD = dg/dD . dD + dg/dx . dx  with dx the field tangent along dD (deff_tangent_rhs_D(dD), then
 * deff_solve_tangent).  Both parts are face-local.
 *
 * deff_sensitivity_hvp_D: hv[p] from the current field x, the current tangent y = dx, D and dD, in one pass.  With dx, dy of
 * deff_mesh, wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), d[p] = (D[p] == 0) ? 0 : dD[p], x, y and d of cell p and of its
 * neighbour q:
 *   interior face of p towards q (weight w = wx for W / E, wy for N / S):
 *       s = Dp + Dq;  tq = (s == 0) ? 0 : Dq / s;  tp = (s == 0) ? 0 : Dp / s;  u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;
 *       e = xp - xq;  f = yp - yq;  c = w * ((4.0 * tq) * (u * (e * e)) + (4.0 * (tq * tq)) * (e * f))
 *   left / right wall:  e = xp - CL (CR);  c = ww * (2.0 * (e * yp))          no face (first / last row of an image):  c = +0.0
 *   hv[p] = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL)),   and hv[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/sens_hvp_model.py states them in numpy; the library is built without contraction).  u is
 * the change of the quotient tq along dD; seen from q it is exactly -u, and e * e and e * f have the same bits from either
 * side, so a face is evaluated once for both cells:  cq = w * ((4.0 * tp) * ((-u) * (e * e)) + (4.0 * (tp * tp)) * (e * f)).
 * Only the sign of a zero can differ from the expressions above, which no comparison of doubles sees.
 * curv[k] = sum over image k of d[p] * hv[p] = dD^T H dD, the curvature of deff_raw along dD, a wave-level reduction in a
 * fixed order (csrc/kernels_facepass.hpp), the same bits on every call.  Checks that need no reference: deff_raw is
 * homogeneous of degree 1 in D, so g is of degree 0 and H D = 0; H is symmetric; and deff_raw is a minimum over fields of
 * functions linear in D, hence concave: curv <= 0 for a converged x and its own dx.  hv (nimg*ny*nx, true width) and curv
 * ([nimg]) may each be NULL; *ms (may be NULL) = device time of the pass, on an event pair of its own.
 *   D and dD [nimg*ny*nx] on the host, as deff_tangent_rhs_D takes them.  The call reads the newest field and the current
 *   tangent dx; that dx belongs to THIS dD (and to this D and field) is the caller's responsibility: the pass cannot tell.
 *   Plain and stack contexts; NULL ctx, D or dD, a row-slab context, CR == CL: DEFF_EINVAL; no field, or no valid tangent:
 *   DEFF_ESTATE.  Pending work is settled first and every image's newest field is read.  The call writes only its own map, its
 *   partial sums and the upload scratch (which holds both planes: 2 n doubles); a refused call leaves the previous map alone.
 *   Negative or non-finite D, dD or dx: unspecified values, never a fault.
 * Tuning "hvp_kt" and deff_get_plan "hvp_kt" / "hvp_items": as "tan_kt" / "tan_items", the same planner.
 * deff_device_sensitivity_hvp: the device buffer of the last map (row pitch as deff_device_field, the pad column of an odd
 *   width holds 0), valid until the next deff_sensitivity_hvp_D or deff_destroy; DEFF_ESTATE before one exists.
 * deff_set_tangent: dx[nimg*ny*nx] (host, true width) becomes the tangent field and is valid -- a caller's own dx, the
 *   counterpart of deff_set_adjoint: for a dx computed elsewhere, and for the pass on arbitrary planes without a solve.  The
 *   same lifetime and invalidation as after deff_solve_tangent; the map's use as a right-hand side is not touched.  Allocates
 *   the tangent's buffer if needed.  NULL arguments and row-slab contexts: DEFF_EINVAL; no system: DEFF_ESTATE.
 * The whole product: deff_tangent_rhs_D(dD), deff_solve_tangent, deff_sensitivity_hvp_D(dD). */
int deff_sensitivity_hvp_D(deff_ctx *ctx, const double *D, const double *dD, double CL, double CR,
                           double *hv /* nimg*ny*nx, may be NULL */, double *curv /* [nimg], may be NULL */, float *ms);
int deff_device_sensitivity_hvp(deff_ctx *ctx, void **d_hv, size_t *row_pitch_bytes);
int deff_set_tangent(deff_ctx *ctx, const double *dx);
/* ---- second-order field adjoint: hv = S_w dD, S_w the Hessian of phi_w(D) = w^T x(D) with the incoming gradient w = dL/dx held
 * fixed, two side solves and one pass (nothing like it in the reference): the term that makes the Gauss-Newton product
 * J^T L'' J of a loss on the field into its Hessian.  g = grad phi_w is deff_field_vjp_D's map, a function of (x, lambda, D);
 * along dD, x moves by y = dx (the field tangent: deff_tangent_rhs_D, deff_solve_tangent), lambda by m = dlambda with
 * A dlambda = -dA lambda =: q, and the quotient tq = Dq / s by u.  All three parts are face-local.
 *
 * deff_adjoint_tangent_rhs_D: q[p] from the current lambda, D and dD: deff_tangent_rhs_D's pass and expressions with lambda in
 *   the place of the field and both wall values 0 (bit for bit tests/tangent_model.tangent_rhs(lambda, D, dD, 0, 0)), into a map
 *   of its own -- deff_device_tangent_rhs's map stays.  norm2[k] = the squared norm of q per image.  q, norm2, ms may be NULL.
 *   Needs a valid lambda (DEFF_ESTATE otherwise); NULL ctx, D or dD and row-slab contexts: DEFF_EINVAL.  Launch geometry: tuning
 *   "tan_kt" (the plan keys "tan_kt" / "tan_items" stay those of the last deff_tangent_rhs_D).  Makes the map a right-hand side
 *   and dlambda invalid.
 * deff_solve_adjoint_tangent: A dlambda = q', q' the map above with the forward system's decoupled rows zeroed, read on the
 *   device; deff_solve_tangent with other buffers, bit for bit the same arithmetic for the same numbers.  Leaves the field,
 *   the system, lambda, dx and every map as they are.  Refusals: those of deff_solve_tangent; DEFF_ESTATE while there is no
 *   right-hand side for the current system and lambda.
 * dlambda's lifetime: deff_solve_adjoint_tangent and deff_set_adjoint_tangent make it valid; every call that invalidates the
 *   adjoint field, and every call that replaces it (deff_solve_adjoint, deff_set_adjoint: a new lambda makes dlambda stale),
 *   invalidates dlambda and the map's use as a right-hand side.  While it is invalid deff_get_adjoint_tangent,
 *   deff_device_adjoint_tangent and deff_field_vjp_hvp_D return DEFF_ESTATE.
 * deff_get_adjoint_tangent / deff_device_adjoint_tangent / deff_set_adjoint_tangent: as deff_get_tangent / deff_device_tangent
 *   / deff_set_tangent (the setter needs a system; it lets the pass run on arbitrary planes).
 *
 * deff_field_vjp_hvp_D: hv[p] from the current field x, lambda l, tangent y, dlambda m, D and dD, in one pass.  With dx, dy of
 * deff_mesh, wx = dy / dx, wy = dx / dy, ww = dy / (dx / 2.0), d[p] = (D[p] == 0) ? 0 : dD[p]:
 *   interior face of p towards q (weight w = wx for W / E, wy for N / S):
 *       s = Dp + Dq;  tq = (s == 0) ? 0 : Dq / s;  tp = (s == 0) ? 0 : Dp / s;  u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;
 *       e = xp - xq;  fl = lp - lq;  ed = yp - yq;  fm = mp - mq;  ef = e * fl;  k = ed * fl + e * fm;
 *       c = w * ((4.0 * tq) * (u * ef) + (2.0 * (tq * tq)) * k)
 *   left / right wall:  e = xp - CL (CR);  c = ww * (yp * lp + e * mp)        no face (first / last row of an image):  c = +0.0
 *   hv[p] = -(((cW + cE) + cN) + cS),   and hv[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/field_hvp_model.py states them in numpy; the library is built without contraction).
 * Seen from q, u is exactly -u and ef, k have the same bits, so a face is evaluated once for both cells:
 *   cq = w * ((4.0 * tp) * ((-u) * ef) + (2.0 * (tp * tp)) * k).  Only the sign of a zero can differ from the expressions above.
 * curv[k] = sum over image k of d[p] * hv[p] = dD^T S_w dD, a wave-level reduction in a fixed order
 * (csrc/kernels_facepass.hpp), the same bits on every call; it has no sign.  Checks that need no reference: phi_w is
 * homogeneous of degree 0 in D, so g is of degree -1 and S_w D = -g; S_w is symmetric; S_w is linear in w.  hv (nimg*ny*nx,
 * true width) and curv ([nimg]) may each be NULL; *ms (may be NULL) = device time of the pass, on an event pair of its own.
 *   D and dD [nimg*ny*nx] on the host.  CR == CL is allowed (nothing is divided by it).  That lambda, dx and dlambda belong to
 *   THIS dD, D and field is the caller's responsibility: the pass cannot tell.
 *   Plain and stack contexts; NULL ctx, D or dD, a row-slab context: DEFF_EINVAL; no field, no valid lambda, no valid tangent,
 *   no valid dlambda: DEFF_ESTATE, the message names which.  The call writes only its own map, its partial sums and the upload
 *   scratch (2 n doubles); a refused call leaves the previous map alone.  Non-finite planes: unspecified values, never a fault.
 * Tuning "fhvp_kt" and deff_get_plan "fhvp_kt" / "fhvp_items": as "hvp_kt" / "hvp_items", the same planner.
 * deff_device_field_vjp_hvp: the device buffer of the last map (row pitch as deff_device_field, the pad column of an odd width
 *   holds 0), valid until the next deff_field_vjp_hvp_D or deff_destroy; DEFF_ESTATE before one exists.
 * The whole product, on a converged field with a valid lambda: deff_tangent_rhs_D(dD), deff_solve_tangent,
 *   deff_adjoint_tangent_rhs_D(dD), deff_solve_adjoint_tangent, deff_field_vjp_hvp_D(dD). */
int deff_adjoint_tangent_rhs_D(deff_ctx *ctx, const double *D, const double *dD,
                               double *q /* nimg*ny*nx, may be NULL */, double *norm2 /* [nimg], may be NULL */, float *ms);
int deff_solve_adjoint_tangent(deff_ctx *ctx, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out /* [nimg] */);
int deff_get_adjoint_tangent(deff_ctx *ctx, double *dl);
int deff_device_adjoint_tangent(deff_ctx *ctx, void **d_dl, size_t *row_pitch_bytes);
int deff_set_adjoint_tangent(deff_ctx *ctx, const double *dl);
int deff_field_vjp_hvp_D(deff_ctx *ctx, const double *D, const double *dD, double CL, double CR,
                         double *hv /* nimg*ny*nx, may be NULL */, double *curv /* [nimg], may be NULL */, float *ms);
int deff_device_field_vjp_hvp(deff_ctx *ctx, void **d_hv, size_t *row_pitch_bytes);
/* sweep-kernel launches issued by the last deff_sweeps()/deff_solve() and the sweeps one
 * temporally blocked launch performs (1 for the single-sweep kernels).  A chained launch of the streaming kernel
 * (deff_get_plan "tb_chain" = 1: several passes of *sweeps_per_pass sweeps in one launch) counts its PASSES, so that
 * *launches stays nsweeps / T + nsweeps % T there and time / *launches stays the time of one pass. */
int deff_last_launches(const deff_ctx *ctx, int64_t *launches, int *sweeps_per_pass);

/* ---- row slabs: ONE image split over several GPUs (BASELINE config #4; nothing like it in the
 * reference, which is pinned to device 0, cuh:908).  Slab r owns a contiguous block of rows and
 * keeps 8 halo rows on each side; one neighbour exchange per temporally blocked pass keeps them
 * valid; results are bit-identical to the one-GPU path.  This group form drives all slabs from
 * one process (devices[r] may repeat: N slabs on one GPU is how the path is tested on one GPU). */
typedef struct deff_slab_group deff_slab_group;
int deff_slab_group_create(int nslabs, const int *devices, int nx, int NY, deff_slab_group **out);
int deff_slab_group_destroy(deff_slab_group *g);
int deff_slab_group_layout(const deff_slab_group *g, int *first_row, int *row_count);
int deff_slab_group_set_tuning(deff_slab_group *g, const char *key, int value);
/* deff_get_plan() of slab `slab`: every slab of an image plans the same sweeps-per-pass ("tb_T") */
int deff_slab_group_get_plan(deff_slab_group *g, int slab, const char *key, int *value);
int deff_slab_group_set_image(deff_slab_group *g, const uint8_t *pix /* NY*nx */);
int deff_slab_group_synth_image(deff_slab_group *g, uint64_t seed, uint64_t img);
int deff_slab_group_assemble_2phase(deff_slab_group *g, double Ds, double Df, double CL, double CR);
/* 3-phase system (deff_assemble_3phase per slab); Grid = flood-fill result of the whole image, NY*nx, or NULL */
int deff_slab_group_assemble_3phase(deff_slab_group *g, double Ds, double Df, double Dg, const unsigned int *Grid,
                                    double CL, double CR);
int deff_slab_group_init_linear(deff_slab_group *g, double CL, double CR);
int deff_slab_group_set_field(deff_slab_group *g, const double *x /* NY*nx */);
int deff_slab_group_get_field(deff_slab_group *g, double *x /* NY*nx */);
int deff_slab_group_sweeps(deff_slab_group *g, int64_t n, double omega, float *ms);
int deff_slab_group_flux(deff_slab_group *g, double *deff_raw, double *MFL, double *MFR);
int deff_slab_group_solve(deff_slab_group *g, double omega, double tol, int64_t max_iter,
                          int64_t check_every, deff_result *out, double *MFL, double *MFR);
/* deff_solve_cg for the image the slabs hold: the current field is the guess and the solution is written into it; the same
 * recurrence, the same stop rules decided on the device (||r|| <= rtol ||b||, max_iter, breakdown), the same true-residual
 * round at the end with up to 8 restart rounds; rel_residual is recomputed from the field and `converged` derived from it;
 * deff_raw / MFL / MFR (NY each, may be NULL) are deff_slab_group_flux of the returned field; loop_ms is slab 0's stream time
 * with the other slabs waited for.  Same argument checks and the same admissibility rules (a row dictionary in every slab,
 * no wall link into the neighbouring row, finite A0 > 0, symmetric links -- checked on the device over each slab's rows):
 * DEFF_EINVAL otherwise, DEFF_ESTATE for a slab without a field or without wall diffusivities, as deff_solve_cg gives them.
 * Every slab's verdict is gathered before anything is written, so all slabs refuse or none; on a refusal no slab's field
 * is changed and deff_slab_group_get_plan reports what it reported before the call.
 *   Each slab iterates its own rows with slab forms of the streaming kernels.  Per iteration one row of the residual
 * travels to each neighbouring slab and every slab's partial dot products -- reduced per slab in a fixed order -- are
 * gathered and added in slab order ((S0 + S1) + S2) + ... by every slab, so all slabs hold the same alpha, beta and stop
 * decision bit for bit.  The results are deterministic and do not depend on check_every, on the transport or on the group /
 * rank form.  With ONE slab they are the bits of deff_solve_cg on a plain context.  With more, the dot products are
 * grouped by slab: the field agrees with the one-context solve to rounding, not bit for bit (as the on-chip form does).
 * The tuning key "cg_onchip" has no effect.  deff_slab_group_get_plan, per slab: "cg_kr" and "cg_strips" (from the whole
 * image, the same on every slab), "cg_items" (this slab's work items), "cg_restarts", "cg_impl" = 1.
 *   After DEFF_OK the group is an ordinary slab set: all 8 halo rows of every slab's current field hold the neighbours'
 * rows, as after deff_slab_group_set_field. */
int deff_slab_group_solve_cg(deff_slab_group *g, double rtol, int64_t max_iter, int64_t check_every,
                             deff_cg_result *out /* [1] */, double *MFL, double *MFR);

/* ---- row slabs, one process per GPU: same slabs, RCCL transport (grouped ncclSend/ncclRecv of the
 * 8-row halo blocks between neighbour ranks once per blocked pass; ncclAllGather of the per-row
 * wall fluxes at a check).  Rank 0 makes the 128-byte id with deff_rccl_unique_id() and hands it
 * to the others (torch.distributed broadcast, a file, MPI ...).  solve/sweeps are collective. */
typedef struct deff_slab_rank deff_slab_rank;
int deff_rccl_unique_id(char *id128);
int deff_slab_rank_create(int device, int nx, int NY, int rank, int nranks, const char *id128,
                          deff_slab_rank **out);
/* the same slab with a caller-supplied, host-staged transport instead of RCCL (testing, portability):
 *   exchange(user, send_up, recv_up, send_down, recv_down, count): swap `count` doubles with the
 *     rank above (NULL pointers on the first rank) and below (NULL on the last); 0 = ok
 *   allgather(user, mine, all, count): all[r*count ..] = rank r's `mine`; 0 = ok */
typedef int (*deff_host_exchange_fn)(void *user, const double *send_up, double *recv_up, const double *send_down,
                                     double *recv_down, size_t count);
typedef int (*deff_host_allgather_fn)(void *user, const double *mine, double *all, size_t count);
int deff_slab_rank_create_custom(int device, int nx, int NY, int rank, int nranks, deff_host_exchange_fn exchange,
                                 deff_host_allgather_fn allgather, void *user, deff_slab_rank **out);
int deff_slab_rank_destroy(deff_slab_rank *s);
int deff_slab_rank_layout(const deff_slab_rank *s, int *first_row, int *row_count);   /* rows it owns */
int deff_slab_rank_window(const deff_slab_rank *s, int *first_row, int *row_count);   /* rows it holds */
int deff_slab_rank_context(deff_slab_rank *s, deff_ctx **ctx);   /* for set_tuning / assemble_2phase / init_linear */
/* deff_set_tuning() of the slab's context, plus "slab_overlap": the halo exchange of a pass runs on a second stream while
 * the interior of the slab is still being swept -- 0 = never (pass, exchange, pass on one stream), 1 = default: for slabs
 * of 16 Mi cells and more, 2 = always */
int deff_slab_rank_set_tuning(deff_slab_rank *s, const char *key, int value);
int deff_slab_rank_set_image_window(deff_slab_rank *s, const uint8_t *pix_window);
/* 3-phase system of this rank's slab; Grid_window = the rows deff_slab_rank_window() names, or NULL */
int deff_slab_rank_assemble_3phase(deff_slab_rank *s, double Ds, double Df, double Dg, const unsigned int *Grid_window,
                                   double CL, double CR);
int deff_slab_rank_synth_image(deff_slab_rank *s, uint64_t seed, uint64_t img);
int deff_slab_rank_get_field(deff_slab_rank *s, double *x_own);
int deff_slab_rank_sweeps(deff_slab_rank *s, int64_t n, double omega, float *ms);
int deff_slab_rank_solve(deff_slab_rank *s, double omega, double tol, int64_t max_iter,
                         int64_t check_every, deff_result *out, double *MFL, double *MFR);
/* deff_slab_group_solve_cg, one process per slab; collective like deff_slab_rank_solve: every rank calls it with the same
 * arguments and gets the same result, bit for bit that of a group of as many slabs.  RCCL: per iteration a grouped
 * ncclSend / ncclRecv of one row per neighbour and two ncclAllGather of 3 doubles per rank, on the context's stream, with
 * no host wait inside an interval of check_every iterations.  Custom transport: `exchange` with count = the row pitch (nx
 * rounded up to even) and `allgather` with count = 3, host staged, waiting every time (tests, portability).
 *   A refusal (DEFF_EINVAL, DEFF_ESTATE) and a failed allocation of the work vectors (DEFF_ENOMEM) on any rank travel with
 * the first all-gather, and every rank returns that status.  A rank on which a HIP or RCCL call or a custom callback fails
 * returns at once (DEFF_EHIP, DEFF_ECOMM) and takes no further part: the other ranks then wait in their next collective,
 * as in deff_slab_rank_solve, and the caller has to tear the communicator down. */
int deff_slab_rank_solve_cg(deff_slab_rank *s, double rtol, int64_t max_iter, int64_t check_every,
                            deff_cg_result *out, double *MFL, double *MFR);

/* diagnostics: per wave tile of one temporally blocked pass of the streaming kernel two words -- the wall-clock (100 MHz) start,
 * and duration (low 32 bits) | HW_ID[15:0] << 32 | XCC_ID << 48 (where it ran); resident tiles: 12 wall-clock stamps per tile.
 * out = NULL: only *ntiles (the number of word PAIRS out must hold) is set and the field is left alone.  Otherwise the field
 * ADVANCES: by one pass = T sweeps (deff_get_plan "tb_T"), or by three passes = 3 * T sweeps when the plan is resident
 * ("tb_impl" = 2 and "tb_resident" = 1: the 12 stamps of a resident tile cover three passes).  DEFF_ESTATE, field unchanged,
 * when the sweeps do not resolve to DEFF_KERNEL_MATFREE_TB.
 *   A chained streaming plan ("tb_impl" = 1, "tb_chain" = 1) stamps three passes of ONE chained launch: two header words, then
 * 20 per tile -- start, where it ran, and per pass six clocks (neighbours seen, first row consumed, steady-state loop entered,
 * last store issued, stores acknowledged, flag published).  The caller sets the header in `out` before the call: out[0] = the
 * first pass to stamp, out[1] = the passes of the chain (0: out[0] + 3); the field advances by that many passes.
 * DEFF_EINVAL when so many passes are not one launch. */
int deff_debug_tb_stamps(deff_ctx *ctx, double omega, unsigned long long *out, int *ntiles);

/* raw device pointers for zero-copy interop (torch tensors, RCCL): current field, and the byte
 * pitch between rows -- nx*8 for an even nx, (nx+1)*8 for an odd one (device rows are padded to an
 * even number of cells; the pad cell holds 0 and is not part of the mesh) */
int deff_device_field(deff_ctx *ctx, void **d_x, size_t *row_pitch_bytes);
int deff_synchronize(deff_ctx *ctx);

/* ---- volumes: the 7-point system of an nx x ny x nz mesh from a D volume, its CG solve and its Deff (not in the reference,
 * whose README lists a 3-D version as upcoming).  A first milestone: a host D volume goes in, a field converged to
 * ||b - A x||_2 <= rtol ||b||_2, its Deff and the gradient dDeff/dD come out; everything else that exists for images (Jacobi
 * sweeps, voxel images and dictionaries, stacks, the on-chip and folded forms, row slabs, the adjoint, tangent and Hessian
 * passes, the flux field) does not for volumes.
 * A volume is a type of its own: no deff_ctx entry point takes it.
 *   The domain is the unit cube: dx = 1/nx, dy = 1/ny, dz = 1/nz.  The left and right walls (x) are Dirichlet at half a cell
 * (CL, CR); y and z are zero-flux.  Arrays are D[nz][ny][nx]: cell (k, i, j) at (k*ny + i)*nx + j; slice k - 1 is "back" (B),
 * slice k + 1 "front" (F), row i - 1 is N and row i + 1 is S as in 2-D.  The row of a cell, with whm(w1, w2, x1, x2) =
 * (w1 + w2) / (w1/x1 + w2/x2) (cuh:347-360) and every product and quotient evaluated left to right, is DiscretizeMatrix2D's
 * (cuh:815-902) with the face areas of a volume:
 *   x block: kw = whm(dx/2, dx/2, Dp, Dw), ke = whm(dx/2, dx/2, Dp, De); aW = -kw*dy*dz/dx, aE = -ke*dy*dz/dx,
 *     a0 += (ke*dy*dz/dx + kw*dy*dz/dx).  First column: kw = Dp, no aW, a0 += (ke*dy*dz/dx + kw*dy*dz/(dx/2)),
 *     b += CL*kw*dy*dz/(dx/2).  Last column: ke = Dp, no aE, a0 += (ke*dy*dz/(dx/2) + kw*dy*dz/dx), b += CR*ke*dy*dz/(dx/2).
 *   y block: kn = whm(dy/2, dy/2, Dp, Dn), ks = whm(dy/2, dy/2, Ds, Dp); aN = -kn*dx*dz/dy, aS = -ks*dx*dz/dy,
 *     a0 += (kn*dx*dz/dy + ks*dx*dz/dy); the first row of a slice has the S terms alone, the last the N terms alone.
 *   z block: kb = whm(dz/2, dz/2, Dp, Db), kf = whm(dz/2, dz/2, Df, Dp); aB = -kb*dx*dy/dz, aF = -kf*dx*dy/dz,
 *     a0 += (kb*dx*dy/dz + kf*dx*dy/dz); the first slice has the F terms alone, the last the B terms alone; nz = 1 has no z
 *     block, and as x * 1.0 is exact its doubles are those of deff_assemble_from_D on the same D.
 * deff_volume_create: nx, ny >= 2, nz >= 1 and at most 2^31 cells (the width rounded up to even), else DEFF_EINVAL. */
typedef struct deff_volume deff_volume;
int deff_volume_create(int device, int nx, int ny, int nz, deff_volume **out);
int deff_volume_destroy(deff_volume *v);
int deff_volume_mesh(const deff_volume *v, int *nx, int *ny, int *nz, double *dx, double *dy, double *dz);   /* any may be NULL */
/* the system above from D[nz*ny*nx] on the host (true width); also sets the wall diffusivities the flux evaluation reads
 * (column 0 and column nx - 1 of every row).  The field is left as it is. */
int deff_volume_assemble_from_D(deff_volume *v, const double *D, double CL, double CR);
/* the assembled coefficients: A[n*7] = a0, aW, aE, aS, aN, aB, aF per cell, b[n], n = nz*ny*nx; DEFF_ESTATE before an assembly */
int deff_volume_get_system(deff_volume *v, double *A, double *b);
/* the field, x[nz*ny*nx]: as deff_init_linear (the ramp in x of every row), deff_set_field, deff_get_field, deff_device_field
 * (rows of the pitch deff_device_field describes, slice after slice) */
int deff_volume_init_linear(deff_volume *v, double CL, double CR);
int deff_volume_set_field(deff_volume *v, const double *x);
int deff_volume_get_field(deff_volume *v, double *x);
int deff_volume_device_field(deff_volume *v, void **d_x, size_t *row_pitch_bytes);
/* deff_flux on the volume: the wall flux densities of all ny*nz rows (MFL, MFR: ny*nz values each, may be NULL) and
 * *deff_raw = their mean over both walls / (CR - CL), summed in row order */
int deff_volume_flux(deff_volume *v, double *deff_raw, double *MFL, double *MFR);
/* deff_solve_cg on the volume's coefficient planes: the argument checks, the DEFF_ESTATE cases (no field, no system), the
 * stop rule on the device, the results' independence of check_every, the true-residual rounds (up to 8 restarts),
 * rel_residual recomputed from x, decoupled cells (all six links and b zero) at x = 0 and the b = 0 behaviour are
 * deff_solve_cg's; so is the admissibility check before the field is touched, which also compares aB with the back cell's aF
 * and aF with the front cell's aB bit for bit and refuses a z link out of the volume (DEFF_EINVAL; a refusal changes
 * nothing).  out: one result; MFL / MFR: ny*nz values each, may be NULL.  The iteration is the plane form's with the back and
 * front rows added: a volume of one slice gives the bits of deff_solve_cg under "cg_planes" on the same D. */
int deff_volume_solve_cg(deff_volume *v, double rtol, int64_t max_iter, int64_t check_every, deff_cg_result *out,
                         double *MFL, double *MFR);
/* of the last deff_volume_solve_cg: "cg_kr", "cg_items", "cg_restarts" as deff_get_plan gives them for an image of ny*nz rows,
 * and "cg_impl" (5 = the volume form; 0 before a solve); of the last deff_volume_sensitivity_D that launched: "sens_kt" and
 * "sens_items" as deff_get_plan gives them for an image of ny*nz rows; any other key: DEFF_EINVAL */
int deff_volume_get_plan(deff_volume *v, const char *key, int *value);
/* The Deff gradient of the volume's current field, meaningful for a CONVERGED one (deff_volume_solve_cg): g[p] = d deff_raw /
 * d D[p] for every cell, in one pass over the field and the diffusivities, no second solve (deff_sensitivity_D's derivation:
 * the system is self-adjoint, and the volume's Deff is 2E / (CR - CL)^2 because wall area and length of the unit cube are 1).
 * Face weights, each evaluated left to right: wx = dy * dz / dx for W / E faces, wy = dx * dz / dy for N / S faces,
 * wz = dx * dy / dz for B / F faces, ww = dy * dz / (dx / 2.0) for the two walls.  Each face of cell p adds
 *   interior, to q:  s = Dp + Dq;  t = (s == 0) ? 0 : Dq / s;  e = xp - xq;  c = (2.0 * (t * t)) * (w * (e * e))
 *   left / right wall:  e = xp - CL (CR);  c = ww * (e * e)
 *   no face (the first and last row of every slice, the first and last slice):  c = +0.0
 *   g[p] = (((((cW + cE) + cN) + cS) + cB) + cF) / ((CR - CL) * (CR - CL)),  and g[p] = 0 where D[p] == 0.
 * These doubles, in this order (tests/volume_sens_model.py states them in numpy); x * 1.0 is exact, so a volume of one slice
 * gives the bits of deff_sensitivity_D.  euler = sum over the cells of D[p] * g[p], which equals deff_raw for the exact
 * solution, added in deff_sensitivity_D's fixed order over the image of ny*nz rows: the same bits on every call.
 *   D[nz*ny*nx] on the host (true width), as deff_volume_assemble_from_D takes it.  g (nz*ny*nx, true width), euler (one
 * double) and *ms (device time of the pass, on an event pair of its own) may each be NULL.  The map is a function of any
 * field: no system is needed.  Refused before anything is touched, in this order: a NULL volume, a NULL D (DEFF_EINVAL), no
 * field (DEFF_ESTATE), CR == CL (DEFF_EINVAL).  Nothing changes but the map, its partial sums and the upload scratch; a refused
 * call leaves the previous map alone.  Negative or non-finite D: unspecified values, never a fault.
 * deff_volume_device_sensitivity: the device buffer of the last map (row pitch as deff_volume_device_field, slice after
 * slice), valid until the next sensitivity call or deff_volume_destroy; DEFF_ESTATE before one exists.
 * deff_volume_set_tuning: "sens_kt" -- tiles of 8 rows one wave streams through (0 = the planner's choice, clipped to the
 * image of ny*nz rows) -- and no other key (DEFF_EINVAL, the key named). */
int deff_volume_sensitivity_D(deff_volume *v, const double *D, double CL, double CR,
                              double *g /* nz*ny*nx, may be NULL */, double *euler /* may be NULL */, float *ms);
int deff_volume_device_sensitivity(deff_volume *v, void **d_g, size_t *row_pitch_bytes);
int deff_volume_set_tuning(deff_volume *v, const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif /* DEFF_AMD_H */
