"""Host-side wrapper of one solver context (one GPU, one mesh).

Thin: every method is one call into the C ABI (include/deff_amd.h).  Array
conventions are the reference's: row-major (ny, nx) fields, A as (n, 5) =
P, W, E, S(row+1), N(row-1) (Deff2D.cuh:815-902).
"""
import collections
import ctypes as C

import numpy as np

from . import _capi
from ._capi import KERNEL_NAMES, CGResultC, DeffError, Result, check

OMEGA_REFERENCE = 2.0 / 3.0     # updateX_SOR, Deff2D.cuh:72


class SolveResult:
    __slots__ = ("iters", "checks", "deff_raw", "conv", "loop_ms", "MFL", "MFR", "field", "slot")

    def __repr__(self):
        return (f"SolveResult(iters={self.iters}, checks={self.checks}, deff_raw={self.deff_raw!r}, "
                f"conv={self.conv!r}, loop_ms={self.loop_ms:.3f})")


class CGResult:
    """deff_solve_cg of one image: CG iterations, ||b - A x|| / ||b|| recomputed from the returned field, its Deff (not / Df)."""
    __slots__ = ("iters", "rel_residual", "deff_raw", "converged", "loop_ms", "MFL", "MFR", "field", "slot")

    def __repr__(self):
        return (f"CGResult(iters={self.iters}, rel_residual={self.rel_residual!r}, deff_raw={self.deff_raw!r}, "
                f"converged={self.converged}, loop_ms={self.loop_ms:.3f})")


def _slab_solve_cg(fn, handle, ny, rtol, max_iter, check_every, fluxes):
    """deff_slab_group_solve_cg / deff_slab_rank_solve_cg -> CGResult with the image's NY wall fluxes."""
    res = CGResultC()
    MFL = np.zeros(ny)
    MFR = np.zeros(ny)
    check(fn(handle, float(rtol), int(max_iter), int(check_every), C.byref(res),
             MFL.ctypes.data_as(C.c_void_p) if fluxes else None, MFR.ctypes.data_as(C.c_void_p) if fluxes else None))
    out = CGResult()
    out.iters, out.rel_residual, out.deff_raw = res.iters, res.rel_residual, res.deff_raw
    out.converged, out.loop_ms = bool(res.converged), res.loop_ms
    out.MFL, out.MFR = MFL, MFR
    return out


FluxField = collections.namedtuple("FluxField", "fx fy left sections")


def flux_vectors(ff, nx, ny):
    """Cell-centred physical flux densities (Jx, Jy) of a FluxField of ONE image (or one image of a stack: fx, fy (ny, nx), left
    (ny,)), numpy only: Jx = -(fxW + fx) / (2 dy), Jy = -(fyN + fy) / (2 dx) with dx = 1 / nx, dy = 1 / ny, fxW the east flux
    of the west neighbour (left in column 0) and fyN the south flux of the north neighbour (0 in row 0).  The face fluxes are
    "higher index minus lower" and integrated over the face, hence the sign and the division by the face's length."""
    fx = np.asarray(ff.fx, dtype=np.float64).reshape(ny, nx)
    fy = np.asarray(ff.fy, dtype=np.float64).reshape(ny, nx)
    left = np.asarray(ff.left, dtype=np.float64).reshape(ny)
    dx, dy = 1.0 / nx, 1.0 / ny
    fxW = np.concatenate([left[:, None], fx[:, :-1]], axis=1)
    fyN = np.concatenate([np.zeros((1, nx)), fy[:-1, :]], axis=0)
    return -(fxW + fx) / (2 * dy), -(fyN + fy) / (2 * dx)


def recommended_batch(nx, ny, images, device=0):
    """Slots a stack Solver(nx, ny, nimg=...) should have to solve `images` images (deff_recommended_batch)."""
    n = C.c_int()
    check(_capi.load().deff_recommended_batch(int(device), int(nx), int(ny), int(images), C.byref(n)))
    return n.value


class Solver:
    """One context: `nimg` images of an nx x ny mesh (nimg > 1 = dataset-generation batch,
    arrays are then stacked image after image: shape (nimg*ny, nx))."""

    def __init__(self, nx, ny, device=0, kernel="auto", nimg=1):
        self._L = _capi.load()
        self._ctx = C.c_void_p()
        self.nx, self.ny, self.nimg = int(nx), int(ny), int(nimg)
        self.rows = self.ny * self.nimg
        check(self._L.deff_create_batch(int(device), self.nx, self.ny, self.nimg, C.byref(self._ctx)))
        if kernel != "auto":
            self.set_kernel(kernel)

    # -- lifecycle --------------------------------------------------------
    def close(self):
        if self._ctx:
            self._L.deff_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel(self, kernel):
        k = KERNEL_NAMES[kernel] if isinstance(kernel, str) else int(kernel)
        check(self._L.deff_set_kernel(self._ctx, k))

    def kernel_in_use(self):
        k = C.c_int()
        check(self._L.deff_get_kernel(self._ctx, C.byref(k)))
        return {v: n for n, v in KERNEL_NAMES.items()}[k.value]

    def set_tuning(self, key, value):
        check(self._L.deff_set_tuning(self._ctx, key.encode(), int(value)))

    def plan(self):
        """What the temporally blocked kernel's last launch plan chose (zeros before any sweep), and "cg_impl": the form of
        the last solve_cg (1 streaming kernels, 2 one image per compute unit: set_tuning("cg_onchip", 1), 3 on the coefficient
        planes: set_tuning("cg_planes", 1 or 2), 4 one image per compute unit on the coefficient planes:
        set_tuning("cg_onchip_planes", 1); 0 before one).  "prescaled": 1 when the last sweeps ran the pre-scaled five-FMA
        arithmetic (set_tuning("prescaled", 1): opt-in, not bit-identical to the reference's written order)."""
        out = {}
        for key in ("tb_T", "tb_LY", "tb_strips", "tb_chunks_per_image", "tb_blocks", "tb_impl", "tb_R", "tb_NW", "tb_resident", "tb_sym", "tb_ranked", "tb_aged", "cg_impl", "prescaled"):
            v = C.c_int()
            check(self._L.deff_get_plan(self._ctx, key.encode(), C.byref(v)))
            out[key] = v.value
        return out

    def plan_value(self, key):
        """One key of deff_get_plan, e.g. "tb_fallbacks" (resident intervals that were redone with one launch per pass)."""
        v = C.c_int()
        check(self._L.deff_get_plan(self._ctx, key.encode(), C.byref(v)))
        return v.value

    # -- image / assembly -------------------------------------------------
    def set_image(self, pix, ampX=1, ampY=1):
        pix = np.ascontiguousarray(pix, dtype=np.uint8)
        if pix.ndim == 3:                                   # (nimg, H, W)
            assert pix.shape[0] == self.nimg
            H, W = pix.shape[1:]
        else:                                               # (nimg*H, W)
            assert pix.shape[0] % self.nimg == 0
            H, W = pix.shape[0] // self.nimg, pix.shape[1]
        check(self._L.deff_set_image(self._ctx, pix.reshape(-1, W), W, H, ampX, ampY))

    def synth_image(self, seed=12345, img=0):
        check(self._L.deff_synth_image(self._ctx, seed, img))

    def get_image(self):
        out = np.empty((self.rows, self.nx), dtype=np.uint8)   # only valid for amp 1
        check(self._L.deff_get_image(self._ctx, out))
        return out

    def assemble_2phase(self, Ds, Df, CL, CR):
        check(self._L.deff_assemble_2phase(self._ctx, Ds, Df, CL, CR))

    def assemble_3phase(self, Ds, Df, Dg, CL, CR, grid=None):
        g = None
        if grid is not None:
            grid = np.ascontiguousarray(grid, dtype=np.uint32)
            assert grid.size == self.nx * self.rows
            g = grid.ctypes.data_as(C.c_void_p)
        check(self._L.deff_assemble_3phase(self._ctx, Ds, Df, Dg, g, CL, CR))

    def assemble_3phase_native(self, Ds, Df, Dg, CL, CR):
        """The 3-phase system with the flood-filled Grid, assembled on the device from the pixels: flood fill on bitmaps, row
        codes, an a-priori table of 452 rows.  A further call on the same image (a continuation stage) rebuilds the table only."""
        check(self._L.deff_assemble_3phase_native(self._ctx, Ds, Df, Dg, CL, CR))

    def grid(self):
        """The device fill of the current image: (grid[nimg*ny, nx] uint32 in FloodFill's encoding, path[nimg] bool)."""
        g = np.empty((self.rows, self.nx), dtype=np.uint32)
        path = np.zeros(self.nimg, dtype=np.int32)
        check(self._L.deff_get_grid(self._ctx, g.ctypes.data_as(C.c_void_p), path.ctypes.data_as(C.c_void_p)))
        return g, path.astype(bool)

    def assemble_from_D(self, D, CL, CR, grid=None):
        D = np.ascontiguousarray(D, dtype=np.float64)
        g = None
        if grid is not None:
            grid = np.ascontiguousarray(grid, dtype=np.uint32)
            g = grid.ctypes.data_as(C.c_void_p)
        check(self._L.deff_assemble_from_D(self._ctx, D, g, CL, CR))

    def set_system(self, A, b, D, CL, CR):
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        d = None
        if D is not None:
            D = np.ascontiguousarray(D, dtype=np.float64)
            d = D.ctypes.data_as(C.c_void_p)
        check(self._L.deff_set_system(self._ctx, A, b, d, CL, CR))

    def get_system(self):
        n = self.nx * self.rows
        A = np.empty((n, 5), dtype=np.float64)
        b = np.empty(n, dtype=np.float64)
        check(self._L.deff_get_system(self._ctx, A, b))
        return A, b

    def dictionary(self):
        """(rows, codes) of the matrix-free form (deff_get_dictionary): rows (R, 6) = a0, aW, aE, aS, aN, b with row 0 the
        zero row, codes (nimg*ny, pitch) uint16 = 8 x each cell's row index, pitch = nx rounded up to even (the pad column of
        an odd width included).  Harvested and a-priori tables alike; DeffError (DEFF_ESTATE) without a matrix-free form.
        A harvested table is ordered by population, ties by the rows' bit patterns: plan_value("dict_outcome") says how the
        harvest ended (0 none tried, 1 harvested, 2 too many rows, 3 hash table overflow, 4 mismatch), "dict_rows" how many
        rows it found."""
        nrows = self.plan_value("lut_rows")
        if nrows == 0:
            check(self._L.deff_get_dictionary(self._ctx, None, None))   # raises: the library's own refusal
        rows = np.empty((nrows, 6), dtype=np.float64)
        codes = np.empty((self.rows, self.nx + (self.nx & 1)), dtype=np.uint16)
        check(self._L.deff_get_dictionary(self._ctx, rows.ctypes.data_as(C.c_void_p), codes.ctypes.data_as(C.c_void_p)))
        return rows, codes

    # -- field ------------------------------------------------------------
    def init_linear(self, CL, CR):
        check(self._L.deff_init_linear(self._ctx, CL, CR))

    def set_field(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.nx * self.rows
        check(self._L.deff_set_field(self._ctx, x))

    def get_field(self):
        x = np.empty((self.rows, self.nx), dtype=np.float64)
        check(self._L.deff_get_field(self._ctx, x))
        return x

    # -- solve ------------------------------------------------------------
    def solve(self, tol, max_iter, omega=OMEGA_REFERENCE, check_every=10000, fluxes=True):
        """One image: a SolveResult.  Batch: a list with one SolveResult per image (MFL/MFR
        are that image's rows; fluxes=False passes NULL for them, as a caller that only wants Deff does)."""
        res = (Result * self.nimg)()
        MFL = np.zeros(self.rows)
        MFR = np.zeros(self.rows)
        check(self._L.deff_solve_batch(self._ctx, omega, tol, int(max_iter), int(check_every), res,
                                       MFL.ctypes.data_as(C.c_void_p) if fluxes else None,
                                       MFR.ctypes.data_as(C.c_void_p) if fluxes else None))
        outs = []
        for k in range(self.nimg):
            out = SolveResult()
            out.iters, out.checks = res[k].iters, res[k].checks
            out.deff_raw, out.conv, out.loop_ms = res[k].deff_raw, res[k].conv, res[k].loop_ms
            out.MFL = MFL[k * self.ny:(k + 1) * self.ny]
            out.MFR = MFR[k * self.ny:(k + 1) * self.ny]
            outs.append(out)
        return outs[0] if self.nimg == 1 else outs

    def solve_cg(self, rtol=1e-10, max_iter=1_000_000, check_every=64, fluxes=True):
        """Jacobi-preconditioned conjugate gradients from the current field to ||b - A x|| <= rtol ||b|| (deff_solve_cg):
        not the reference's algorithm, the same fixed point.  One image: a CGResult; a stack: a list, one per image.
        A system without a row dictionary (a D plane that varies cell by cell, a caller's set_system, more distinct rows than
        a dictionary holds, set_tuning("dict", 0)) is refused unless set_tuning("cg_planes", 1) lets the iteration read the
        explicit coefficient planes; set_tuning("cg_planes", 2) takes that form for every system (the bits of the table
        form where a dictionary exists).  plan_value("cg_impl") is 3 after such a call.  Explicit-only systems (a wall link
        into the neighbouring row) and row slabs stay refused.
        set_tuning("cg_onchip_planes", 1) (0 or 1; anything else raises DeffError) lets a call that takes the plane form
        iterate images of at most 16 384 cells (pitch x ny) on one compute unit each, as "cg_onchip" does for the table form:
        plan_value("cg_impl") is 4 then, and a system that has a dictionary gets the bits of "cg_onchip" 1.  The key also
        applies to solve_adjoint, solve_tangent and solve_adjoint_tangent, which always run on the planes.
        set_tuning("cg_fold", 1) makes an iteration of the streaming forms (cg_impl 1 and 3) two launches instead of four: the
        per-image sums are taken by the last workgroup to arrive; 2 also lets the table form's direction kernel load a row
        ahead.  The results are those of 0 bit for bit; plan_value("cg_fold") is what the last call ran (0 on chip)."""
        res = (CGResultC * self.nimg)()
        MFL = np.zeros(self.rows)
        MFR = np.zeros(self.rows)
        check(self._L.deff_solve_cg(self._ctx, float(rtol), int(max_iter), int(check_every), res,
                                    MFL.ctypes.data_as(C.c_void_p) if fluxes else None,
                                    MFR.ctypes.data_as(C.c_void_p) if fluxes else None))
        outs = []
        for k in range(self.nimg):
            out = CGResult()
            out.iters, out.rel_residual, out.deff_raw = res[k].iters, res[k].rel_residual, res[k].deff_raw
            out.converged, out.loop_ms = bool(res[k].converged), res[k].loop_ms
            out.MFL = MFL[k * self.ny:(k + 1) * self.ny]
            out.MFR = MFR[k * self.ny:(k + 1) * self.ny]
            outs.append(out)
        return outs[0] if self.nimg == 1 else outs

    def solve_stream(self, images, Ds, Df, CL, CR, tol, max_iter, omega=OMEGA_REFERENCE, check_every=10000,
                     want_fields=False, ampX=1, ampY=1):
        """Dataset generation: `images` is any iterable of uint8 (H, W) arrays of one size; the nimg
        slots of this context are kept full (a finished image's slot is refilled with the next one).
        Returns a list with one SolveResult per image, in input order, with .slot = the slot the image ran in (plus .field
        when want_fields).  Afterwards slot k of the context holds the last image that ran in it, with its final field."""
        it = iter(images)
        H, W = self.ny // ampY, self.nx // ampX
        results = {}
        counter = [0]
        errors = []

        def _next(_user, _slot, pix_ptr, id_ptr):
            try:
                img = next(it)
            except StopIteration:
                return 0
            except Exception as e:          # noqa: BLE001 - reported to the C side as an error code
                errors.append(e)
                return -1
            a = np.ascontiguousarray(img, dtype=np.uint8)
            if a.shape != (H, W):
                errors.append(ValueError(f"image {counter[0]} is {a.shape}, expected {(H, W)}"))
                return -1
            C.memmove(pix_ptr, a.ctypes.data, a.size)
            id_ptr[0] = counter[0]
            counter[0] += 1
            return 1

        def _done(_user, image_id, slot, res_ptr):
            # an exception raised inside a ctypes callback is swallowed: record it, re-raise after the call
            try:
                r = res_ptr[0]
                out = SolveResult()
                out.iters, out.checks, out.deff_raw, out.conv, out.loop_ms = r.iters, r.checks, r.deff_raw, r.conv, r.loop_ms
                out.MFL = out.MFR = None
                out.slot = int(slot)
                if want_fields:
                    x = np.empty((self.ny, self.nx), dtype=np.float64)
                    check(self._L.deff_get_slot_field(self._ctx, slot, x))
                    out.field = x
                results[int(image_id)] = out
            except Exception as e:          # noqa: BLE001
                errors.append(e)

        nxt, dn = _capi.NEXT_IMAGE_FN(_next), _capi.IMAGE_DONE_FN(_done)
        rc = self._L.deff_solve_stream(self._ctx, W, H, ampX, ampY, Ds, Df, CL, CR, omega, tol, int(max_iter),
                                       int(check_every), nxt, dn, None)
        if errors:
            raise errors[0]
        check(rc)
        return [results[k] for k in range(counter[0])]

    def solve_cg_stream(self, images, Ds, Df, CL, CR, rtol=1e-10, max_iter=1_000_000, check_every=64, want_fields=False,
                        ampX=1, ampY=1):
        """solve_stream with conjugate gradients (deff_solve_cg_stream): every image of the iterable is solved to
        ||b - A x|| <= rtol ||b|| from the linear guess, exactly as a one-image solve_cg would, in whichever slot is free.
        Returns a list with one CGResult per image, in input order, with .slot (plus .field when want_fields; MFL / MFR are
        None).  Afterwards slot k of the context holds the last image that ran in it, with its final field.
        With set_tuning("cg_fold", 1 or 2) the streaming kernels run two launches per iteration, as in solve_cg (the same
        bits; plan_value("cgs_launches") drops by two per enqueued iteration); images that iterate on chip are not affected."""
        it = iter(images)
        H, W = self.ny // ampY, self.nx // ampX
        results = {}
        counter = [0]
        errors = []

        def _next(_user, _slot, pix_ptr, id_ptr):
            try:
                img = next(it)
            except StopIteration:
                return 0
            except Exception as e:          # noqa: BLE001 - reported to the C side as an error code
                errors.append(e)
                return -1
            a = np.ascontiguousarray(img, dtype=np.uint8)
            if a.shape != (H, W):
                errors.append(ValueError(f"image {counter[0]} is {a.shape}, expected {(H, W)}"))
                return -1
            C.memmove(pix_ptr, a.ctypes.data, a.size)
            id_ptr[0] = counter[0]
            counter[0] += 1
            return 1

        def _done(_user, image_id, slot, res_ptr):
            # an exception raised inside a ctypes callback is swallowed: record it, re-raise after the call
            try:
                r = res_ptr[0]
                out = CGResult()
                out.iters, out.rel_residual, out.deff_raw = r.iters, r.rel_residual, r.deff_raw
                out.converged, out.loop_ms = bool(r.converged), r.loop_ms
                out.MFL = out.MFR = None
                out.slot = int(slot)
                if want_fields:
                    x = np.empty((self.ny, self.nx), dtype=np.float64)
                    check(self._L.deff_get_slot_field(self._ctx, slot, x))
                    out.field = x
                results[int(image_id)] = out
            except Exception as e:          # noqa: BLE001
                errors.append(e)

        nxt, dn = _capi.NEXT_IMAGE_FN(_next), _capi.CG_IMAGE_DONE_FN(_done)
        rc = self._L.deff_solve_cg_stream(self._ctx, W, H, ampX, ampY, Ds, Df, CL, CR, float(rtol), int(max_iter),
                                          int(check_every), nxt, dn, None)
        if errors:
            raise errors[0]
        check(rc)
        return [results[k] for k in range(counter[0])]

    def sweeps(self, n, omega=OMEGA_REFERENCE):
        ms = C.c_float()
        check(self._L.deff_sweeps(self._ctx, int(n), omega, C.byref(ms)))
        return ms.value

    def flux(self):
        d = (C.c_double * self.nimg)()
        MFL = np.zeros(self.rows)
        MFR = np.zeros(self.rows)
        check(self._L.deff_flux(self._ctx, d, MFL.ctypes.data_as(C.c_void_p), MFR.ctypes.data_as(C.c_void_p)))
        return (d[0] if self.nimg == 1 else np.array(d[:])), MFL, MFR

    def residual(self, D=None, CL=None, CR=None, timing=False):
        """Residual() cuh:451-494 of the current field (mean |qW - qE + qN - qS| per cell): a float, or one per image.
        D = None: the system assembled from the image; otherwise the diffusivity plane (rows, nx) with the wall values."""
        r = (C.c_double * self.nimg)()
        ms = C.c_float()
        if D is None:
            check(self._L.deff_residual(self._ctx, r, C.byref(ms)))
        else:
            D = np.ascontiguousarray(D, dtype=np.float64)
            assert D.size == self.nx * self.rows
            check(self._L.deff_residual_D(self._ctx, D, float(CL), float(CR), r, C.byref(ms)))
        out = r[0] if self.nimg == 1 else np.array(r[:])
        return (out, ms.value) if timing else out

    # -- helpers of the passes and side solves below ------------------------
    def _plane(self, a):
        """A plane of the stack, (rows, nx), as contiguous float64."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.nx * self.rows
        return a

    def _cell_pass(self, fn, planes, walls, timing):
        """One pass entry point fn(ctx, *planes, *walls, map, sums, ms) -> (map, sums[, ms]): the map as (ny, nx), or (nimg, ny,
        nx) for a stack, the sums a float, or an array."""
        m = np.empty((self.rows, self.nx), dtype=np.float64)
        e = (C.c_double * self.nimg)()
        ms = C.c_float()
        check(fn(self._ctx, *[a.ctypes.data_as(C.c_void_p) for a in planes], *[float(w) for w in walls],
                 m.ctypes.data_as(C.c_void_p), e, C.byref(ms) if timing else None))
        m = m if self.nimg == 1 else m.reshape(self.nimg, self.ny, self.nx)
        sums = e[0] if self.nimg == 1 else np.array(e[:])
        return (m, sums, ms.value) if timing else (m, sums)

    def _side_solve(self, fn, *rhs, rtol, max_iter, check_every):
        """One side solve fn(ctx, *rhs, rtol, max_iter, check_every, results): a CGResult, or a list for a stack."""
        res = (CGResultC * self.nimg)()
        check(fn(self._ctx, *rhs, float(rtol), int(max_iter), int(check_every), res))
        outs = []
        for r in res:
            out = CGResult()
            out.iters, out.rel_residual, out.deff_raw = r.iters, r.rel_residual, r.deff_raw
            out.converged, out.loop_ms = bool(r.converged), r.loop_ms
            out.MFL = out.MFR = None
            outs.append(out)
        return outs[0] if self.nimg == 1 else outs

    def _device_ptr(self, fn):
        """(device pointer, row pitch in bytes) from one of the deff_device_* getters."""
        p = C.c_void_p()
        pitch = C.c_size_t()
        check(fn(self._ctx, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    @staticmethod
    def _require_converged(who, rs, rtol, max_iter):
        rs = rs if isinstance(rs, list) else [rs]
        bad = [k for k, r in enumerate(rs) if not r.converged]
        if bad:
            raise RuntimeError(f"{who}: CG did not converge to rtol {rtol} for image(s) {bad} "
                               f"(rel_residual {[rs[k].rel_residual for k in bad]}, max_iter {max_iter})")

    def _get_plane(self, fn):
        a = np.empty((self.rows, self.nx), dtype=np.float64)
        check(fn(self._ctx, a.ctypes.data_as(C.c_void_p)))
        return a

    def sensitivity(self, D=None, CL=None, CR=None, timing=False):
        """The Deff gradient of the current field (deff_sensitivity / deff_sensitivity_D): (g, euler) with g[p] = d deff_raw /
        d D[p] as (ny, nx), or (nimg, ny, nx) for a stack, and euler = sum of D * g per image (a float, or an array), which
        equals deff_raw for a converged field.  D = None: the diffusivities of the system assembled from the image
        (assemble_2phase, or assemble_3phase without a grid) with its CL, CR; otherwise the plane (rows, nx) with the wall
        values.  timing=True appends the device time in ms."""
        if D is None:
            return self._cell_pass(self._L.deff_sensitivity, (), (), timing)
        return self._cell_pass(self._L.deff_sensitivity_D, (self._plane(D),), (CL, CR), timing)

    def device_sensitivity_ptr(self):
        """(device pointer, row pitch in bytes) of the last sensitivity map; valid until the next one, an assembly or close()."""
        return self._device_ptr(self._L.deff_device_sensitivity)

    # -- flux field: face fluxes and section sums ---------------------------
    def flux_field(self, D=None, CL=None, CR=None, timing=False):
        """The flux through every face of the current field and through every vertical section, in one pass (deff_flux_field /
        deff_flux_field_D): FluxField(fx, fy, left, sections).  fx[p] is the flux through the E face of cell p (the right
        wall's in the last column), fy[p] through its S face (row + 1; +0.0 in an image's last row), both as (ny, nx), or
        (nimg, ny, nx) for a stack; left (nimg, ny) the left wall's; sections (nimg, nx + 1) the sums over the rows of left and
        of every column of fx -- for a converged field all the same number, and (sections[0] + sections[nx]) / (2 (CR - CL))
        is deff_raw.  Sign: "higher index minus lower", the physical flux is the negative (flux_vectors).  D = None: the
        diffusivities of the system assembled from the image (assemble_2phase, or assemble_3phase without a grid) with its CL,
        CR; otherwise the plane (rows, nx).  timing=True appends the device time in ms."""
        fx = np.empty((self.rows, self.nx), dtype=np.float64)
        fy = np.empty((self.rows, self.nx), dtype=np.float64)
        left = np.empty((self.nimg, self.ny), dtype=np.float64)
        sec = np.empty((self.nimg, self.nx + 1), dtype=np.float64)
        ms = C.c_float()
        out = [a.ctypes.data_as(C.c_void_p) for a in (fx, fy, left, sec)] + [C.byref(ms) if timing else None]
        if D is None:
            check(self._L.deff_flux_field(self._ctx, *out))
        else:
            check(self._L.deff_flux_field_D(self._ctx, self._plane(D).ctypes.data_as(C.c_void_p), float(CL), float(CR), *out))
        if self.nimg > 1:
            fx, fy = fx.reshape(self.nimg, self.ny, self.nx), fy.reshape(self.nimg, self.ny, self.nx)
        ff = FluxField(fx, fy, left, sec)
        return ff + (ms.value,) if timing else ff

    def device_flux_field_ptrs(self):
        """(device pointer of fx, device pointer of fy, row pitch in bytes) of the last flux_field maps; valid until the next
        one or close()."""
        px, py = C.c_void_p(), C.c_void_p()
        pitch = C.c_size_t()
        check(self._L.deff_device_flux_field(self._ctx, C.byref(px), C.byref(py), C.byref(pitch)))
        return px.value, py.value, pitch.value

    # -- field adjoint: dL/dD for a loss on the field ----------------------
    def solve_adjoint(self, w, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """A lambda = w on the current matrix with homogeneous walls (deff_solve_adjoint), w = dL/dx as (rows, nx): the
        iteration of solve_cg on the coefficient planes from lambda = 0, into a buffer of the context's own -- the field, the
        system and its dictionary stay as they are.  Cells the forward system decouples ignore w and get lambda = 0.
        With set_tuning("cg_onchip_planes", 1) images of at most 16 384 cells iterate on one compute unit each
        (plan_value("cg_impl") 4), here and in solve_tangent and solve_adjoint_tangent.
        One image: a CGResult (deff_raw 0.0, MFL / MFR None); a stack: a list, one per image."""
        return self._side_solve(self._L.deff_solve_adjoint, self._plane(w).ctypes.data_as(C.c_void_p), rtol=rtol,
                                max_iter=max_iter, check_every=check_every)

    def set_adjoint(self, lam):
        """A caller's own lambda as the adjoint field (deff_set_adjoint)."""
        check(self._L.deff_set_adjoint(self._ctx, self._plane(lam).ctypes.data_as(C.c_void_p)))

    def get_adjoint(self):
        """The adjoint field as (rows, nx); DeffError (DEFF_ESTATE) while none is valid for the current system."""
        return self._get_plane(self._L.deff_get_adjoint)

    def device_adjoint_ptr(self):
        """(device pointer, row pitch in bytes) of the adjoint field; the pitch is device_field_ptr's."""
        return self._device_ptr(self._L.deff_device_adjoint)

    def field_vjp(self, D, CL, CR, timing=False):
        """dL/dD from the current field, the current adjoint field and the diffusivity plane D (rows, nx), in one pass
        (deff_field_vjp_D): (g, euler) with g as (ny, nx), or (nimg, ny, nx) for a stack, and euler = sum of D * g per image
        (a float, or an array), which is 0 for a converged field.  timing=True appends the device time in ms."""
        return self._cell_pass(self._L.deff_field_vjp_D, (self._plane(D),), (CL, CR), timing)

    def device_field_vjp_ptr(self):
        """(device pointer, row pitch in bytes) of the last field_vjp map; valid until the next one or close()."""
        return self._device_ptr(self._L.deff_device_field_vjp)

    # -- field tangent: dx along a direction dD ---------------------------
    def tangent_rhs(self, D, dD, CL, CR, timing=False):
        """r = db - dA x along the direction dD, from the current field and the diffusivity plane D, both (rows, nx), in one
        pass (deff_tangent_rhs_D): (r, norm2) with r as (ny, nx), or (nimg, ny, nx) for a stack, and norm2 = sum of r * r per
        image (a float, or an array); for dD = D it is the forward residual's.  timing=True appends the device time in ms."""
        return self._cell_pass(self._L.deff_tangent_rhs_D, (self._plane(D), self._plane(dD)), (CL, CR), timing)

    def device_tangent_rhs_ptr(self):
        """(device pointer, row pitch in bytes) of the last tangent_rhs map; valid until the next one or close()."""
        return self._device_ptr(self._L.deff_device_tangent_rhs)

    def solve_tangent(self, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """A dx = r on the current matrix with homogeneous walls (deff_solve_tangent), r the last tangent_rhs map, read on the
        device: solve_adjoint's iteration into a buffer of its own -- the field, the system, lambda and the map stay as they
        are.  One image: a CGResult (deff_raw 0.0, MFL / MFR None); a stack: a list, one per image."""
        return self._side_solve(self._L.deff_solve_tangent, rtol=rtol, max_iter=max_iter, check_every=check_every)

    def get_tangent(self):
        """The tangent field dx as (rows, nx); DeffError (DEFF_ESTATE) while none is valid for the current system."""
        return self._get_plane(self._L.deff_get_tangent)

    def device_tangent_ptr(self):
        """(device pointer, row pitch in bytes) of the tangent field; the pitch is device_field_ptr's."""
        return self._device_ptr(self._L.deff_device_tangent)

    def field_jvp(self, D, dD, CL, CR, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """dx = (dx/dD) dD of the current field: tangent_rhs + solve_tangent + get_tangent, as (rows, nx).  RuntimeError if the
        solve does not reach rtol."""
        self._tangent_along("field_jvp", self._plane(D), self._plane(dD), CL, CR, rtol, max_iter, check_every)
        return self.get_tangent()

    def _tangent_along(self, who, D, dD, CL, CR, rtol, max_iter, check_every):
        """tangent_rhs with the map left on the device, then solve_tangent; RuntimeError if the solve does not reach rtol."""
        check(self._L.deff_tangent_rhs_D(self._ctx, D.ctypes.data_as(C.c_void_p), dD.ctypes.data_as(C.c_void_p), float(CL),
                                         float(CR), None, None, None))
        rs = self.solve_tangent(rtol=rtol, max_iter=max_iter, check_every=check_every)
        self._require_converged(who, rs, rtol, max_iter)

    # -- Deff Hessian-vector product: H dD ---------------------------------
    def set_tangent(self, dx):
        """A caller's own dx as the tangent field (deff_set_tangent); needs a system."""
        check(self._L.deff_set_tangent(self._ctx, self._plane(dx).ctypes.data_as(C.c_void_p)))

    def sens_hvp(self, D, dD, CL, CR, timing=False):
        """hv = H dD, H the Hessian of deff_raw with respect to the diffusivity map, from the current field, the current tangent
        field and the planes D and dD, both (rows, nx), in one pass (deff_sensitivity_hvp_D): (hv, curv) with hv as (ny, nx), or
        (nimg, ny, nx) for a stack, and curv = dD^T H dD per image (a float, or an array).  The tangent has to be the one along
        this dD (tangent_rhs + solve_tangent, or set_tangent): deff_hvp does all three.  timing=True appends the device time in
        ms."""
        return self._cell_pass(self._L.deff_sensitivity_hvp_D, (self._plane(D), self._plane(dD)), (CL, CR), timing)

    def device_sens_hvp_ptr(self):
        """(device pointer, row pitch in bytes) of the last sens_hvp map; valid until the next one or close()."""
        return self._device_ptr(self._L.deff_device_sensitivity_hvp)

    def deff_hvp(self, D, dD, CL, CR, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """(hv, curv) = sens_hvp of the current (converged) field along dD with the tangent computed here: tangent_rhs with the
        map left on the device, solve_tangent to rtol (RuntimeError if it does not get there), then sens_hvp.  Overwrites the
        tangent's right-hand side map and the tangent field."""
        D, dD = self._plane(D), self._plane(dD)
        self._tangent_along("deff_hvp", D, dD, CL, CR, rtol, max_iter, check_every)
        return self.sens_hvp(D, dD, CL, CR)

    # -- second-order field adjoint: S_w dD, the Hessian of w^T x(D) -------
    def adjoint_tangent_rhs(self, D, dD, timing=False):
        """q = -dA lambda along the direction dD, from the current adjoint field and the diffusivity plane D, both (rows, nx),
        in one pass (deff_adjoint_tangent_rhs_D: tangent_rhs's pass on lambda with both wall values 0, into a map of its own):
        (q, norm2) with q as (ny, nx), or (nimg, ny, nx) for a stack, and norm2 = sum of q * q per image.  timing=True appends
        the device time in ms."""
        return self._cell_pass(self._L.deff_adjoint_tangent_rhs_D, (self._plane(D), self._plane(dD)), (), timing)

    def solve_adjoint_tangent(self, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """A dlambda = q on the current matrix with homogeneous walls (deff_solve_adjoint_tangent), q the last
        adjoint_tangent_rhs map, read on the device: solve_tangent's iteration into a buffer of its own -- the field, the
        system, lambda, dx and the maps stay as they are.  One image: a CGResult (deff_raw 0.0, MFL / MFR None); a stack: a
        list, one per image."""
        return self._side_solve(self._L.deff_solve_adjoint_tangent, rtol=rtol, max_iter=max_iter, check_every=check_every)

    def get_adjoint_tangent(self):
        """dlambda as (rows, nx); DeffError (DEFF_ESTATE) while none is valid for the current system and adjoint field."""
        return self._get_plane(self._L.deff_get_adjoint_tangent)

    def set_adjoint_tangent(self, dl):
        """A caller's own dlambda (deff_set_adjoint_tangent); needs a system."""
        check(self._L.deff_set_adjoint_tangent(self._ctx, self._plane(dl).ctypes.data_as(C.c_void_p)))

    def device_adjoint_tangent_ptr(self):
        """(device pointer, row pitch in bytes) of dlambda; the pitch is device_field_ptr's."""
        return self._device_ptr(self._L.deff_device_adjoint_tangent)

    def field_vjp_hvp(self, D, dD, CL, CR, timing=False):
        """hv = S_w dD, S_w the Hessian of w^T x(D) with w = A lambda held fixed, from the current field, adjoint field,
        tangent field and dlambda and the planes D and dD, both (rows, nx), in one pass (deff_field_vjp_hvp_D): (hv, curv) with
        hv as (ny, nx), or (nimg, ny, nx) for a stack, and curv = dD^T S_w dD per image (a float, or an array).  The tangent
        and dlambda have to be the ones along this dD: field_hvp does all five steps.  timing=True appends the device time in
        ms."""
        return self._cell_pass(self._L.deff_field_vjp_hvp_D, (self._plane(D), self._plane(dD)), (CL, CR), timing)

    def device_field_vjp_hvp_ptr(self):
        """(device pointer, row pitch in bytes) of the last field_vjp_hvp map; valid until the next one or close()."""
        return self._device_ptr(self._L.deff_device_field_vjp_hvp)

    def field_hvp(self, D, dD, CL, CR, rtol=1e-10, max_iter=1_000_000, check_every=64):
        """(hv, curv) = field_vjp_hvp of the current (converged) field and adjoint field along dD with both tangents computed
        here: tangent_rhs and adjoint_tangent_rhs with their maps left on the device, solve_tangent and solve_adjoint_tangent
        to rtol (RuntimeError if one does not get there), then field_vjp_hvp.  Overwrites both right-hand side maps, the
        tangent field and dlambda."""
        D, dD = self._plane(D), self._plane(dD)
        self._tangent_along("field_hvp", D, dD, CL, CR, rtol, max_iter, check_every)
        check(self._L.deff_adjoint_tangent_rhs_D(self._ctx, D.ctypes.data_as(C.c_void_p), dD.ctypes.data_as(C.c_void_p),
                                                 None, None, None))
        rs = self.solve_adjoint_tangent(rtol=rtol, max_iter=max_iter, check_every=check_every)
        self._require_converged("field_hvp (adjoint tangent)", rs, rtol, max_iter)
        return self.field_vjp_hvp(D, dD, CL, CR)

    def set_progress(self, fn):
        """fn(iter, deff_raw, change) after every convergence check, or None."""
        if fn is None:
            self._progress = _capi.PROGRESS_FN(0)
        else:
            self._progress = _capi.PROGRESS_FN(lambda it, d, ch, _u: fn(it, d, ch))
        check(self._L.deff_set_progress(self._ctx, self._progress, None))

    def last_launches(self):
        """(kernel launches of the last sweeps()/solve(), sweeps per temporally blocked launch)."""
        n = C.c_int64()
        t = C.c_int()
        check(self._L.deff_last_launches(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    def device_field_ptr(self):
        return self._device_ptr(self._L.deff_device_field)

    def synchronize(self):
        check(self._L.deff_synchronize(self._ctx))


class Volume:
    """One nx x ny x nz volume on the unit cube (deff_volume_*): the 7-point system from a per-cell D volume, its CG solve, its
    Deff and the gradient dDeff/dD.  Arrays are (nz, ny, nx); A is (n, 7) = P, W, E, S(row+1), N(row-1), B(slice-1), F(slice+1).  The walls in x are
    Dirichlet (CL, CR), y and z zero-flux.  Nothing else of Solver (the adjoint, tangent and Hessian passes, the flux field)
    exists for volumes yet."""

    def __init__(self, nx, ny, nz, device=0):
        self._L = _capi.load()
        self._vol = C.c_void_p()
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.rows = self.ny * self.nz
        check(self._L.deff_volume_create(int(device), self.nx, self.ny, self.nz, C.byref(self._vol)))

    def close(self):
        if self._vol:
            self._L.deff_volume_destroy(self._vol)
            self._vol = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def mesh(self):
        """(nx, ny, nz, dx, dy, dz)"""
        n = [C.c_int() for _ in range(3)]
        d = [C.c_double() for _ in range(3)]
        check(self._L.deff_volume_mesh(self._vol, *[C.byref(v) for v in n + d]))
        return tuple(v.value for v in n + d)

    def assemble_from_D(self, D, CL, CR):
        D = np.ascontiguousarray(D, dtype=np.float64)
        assert D.size == self.nx * self.rows
        check(self._L.deff_volume_assemble_from_D(self._vol, D, CL, CR))

    def get_system(self):
        n = self.nx * self.rows
        A = np.empty((n, 7), dtype=np.float64)
        b = np.empty(n, dtype=np.float64)
        check(self._L.deff_volume_get_system(self._vol, A, b))
        return A, b

    def init_linear(self, CL, CR):
        check(self._L.deff_volume_init_linear(self._vol, CL, CR))

    def set_field(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.nx * self.rows
        check(self._L.deff_volume_set_field(self._vol, x))

    def get_field(self):
        x = np.empty((self.nz, self.ny, self.nx), dtype=np.float64)
        check(self._L.deff_volume_get_field(self._vol, x))
        return x

    def flux(self):
        """(deff_raw, MFL, MFR): the wall flux densities of all ny * nz rows, slice after slice."""
        d = C.c_double()
        MFL = np.zeros(self.rows)
        MFR = np.zeros(self.rows)
        check(self._L.deff_volume_flux(self._vol, C.byref(d), MFL.ctypes.data_as(C.c_void_p), MFR.ctypes.data_as(C.c_void_p)))
        return d.value, MFL, MFR

    def solve_cg(self, rtol=1e-10, max_iter=1_000_000, check_every=64, fluxes=True):
        """Jacobi-preconditioned conjugate gradients from the current field to ||b - A x|| <= rtol ||b|| (deff_volume_solve_cg):
        Solver.solve_cg's rules on the volume's coefficient planes.  A CGResult with the ny * nz wall fluxes."""
        return _slab_solve_cg(self._L.deff_volume_solve_cg, self._vol, self.rows, rtol, max_iter, check_every, fluxes)

    def plan_value(self, key):
        """"cg_kr", "cg_items", "cg_restarts" or "cg_impl" (5 = the volume form) of the last solve_cg; "sens_kt" or "sens_items"
        of the last sensitivity: the tiles of 8 rows a wave streamed through, and the partial sums added."""
        v = C.c_int()
        check(self._L.deff_volume_get_plan(self._vol, key.encode(), C.byref(v)))
        return v.value

    def set_tuning(self, key, value):
        """"sens_kt": tiles of 8 rows one wave of sensitivity() streams through (0 = the planner's choice); no other key."""
        check(self._L.deff_volume_set_tuning(self._vol, key.encode(), int(value)))

    def sensitivity(self, D, CL, CR, timing=False):
        """The Deff gradient of the current field (deff_volume_sensitivity_D): (g, euler) with g[p] = d deff_raw / d D[p] as
        (nz, ny, nx) and euler = sum of D * g, which equals deff_raw for a converged field.  D: the volume (nz, ny, nx) with
        the wall values.  timing=True appends the device time in ms."""
        D = np.ascontiguousarray(D, dtype=np.float64)
        assert D.size == self.nx * self.rows
        g = np.empty((self.nz, self.ny, self.nx), dtype=np.float64)
        e = C.c_double()
        ms = C.c_float()
        check(self._L.deff_volume_sensitivity_D(self._vol, D.ctypes.data_as(C.c_void_p), float(CL), float(CR),
                                                g.ctypes.data_as(C.c_void_p), C.byref(e), C.byref(ms) if timing else None))
        return (g, e.value, ms.value) if timing else (g, e.value)

    def device_sensitivity_ptr(self):
        """(device pointer, row pitch in bytes) of the last sensitivity map; valid until the next one or close()."""
        p = C.c_void_p()
        pitch = C.c_size_t()
        check(self._L.deff_volume_device_sensitivity(self._vol, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    def device_field_ptr(self):
        p = C.c_void_p()
        pitch = C.c_size_t()
        check(self._L.deff_volume_device_field(self._vol, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value


class SlabGroup:
    """One image split into row slabs over `devices` (one slab per entry; entries may repeat,
    which is how the multi-GPU path is exercised on a single GPU).  Same call sequence as Solver."""

    def __init__(self, nx, NY, devices):
        self._L = _capi.load()
        self._g = C.c_void_p()
        self.nx, self.ny, self.nslabs = int(nx), int(NY), len(devices)
        dev = (C.c_int * len(devices))(*devices)
        check(self._L.deff_slab_group_create(len(devices), dev, self.nx, self.ny, C.byref(self._g)))

    def close(self):
        if self._g:
            self._L.deff_slab_group_destroy(self._g)
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def layout(self):
        a = (C.c_int * self.nslabs)()
        b = (C.c_int * self.nslabs)()
        check(self._L.deff_slab_group_layout(self._g, a, b))
        return list(a), list(b)

    def set_tuning(self, key, value):
        check(self._L.deff_slab_group_set_tuning(self._g, key.encode(), int(value)))

    def plans(self):
        """Every slab's last temporally blocked launch plan (Solver.plan() per slab)."""
        out = []
        for r in range(self.nslabs):
            d = {}
            for key in ("tb_T", "tb_LY", "tb_strips", "tb_chunks_per_image", "tb_blocks", "tb_impl", "tb_R", "tb_NW", "tb_resident", "tb_sym"):
                v = C.c_int()
                check(self._L.deff_slab_group_get_plan(self._g, r, key.encode(), C.byref(v)))
                d[key] = v.value
            out.append(d)
        return out

    def plan_value(self, slab, key):
        """One figure of slab `slab`'s last plan (deff_slab_group_get_plan), e.g. "cg_kr", "cg_items"."""
        v = C.c_int()
        check(self._L.deff_slab_group_get_plan(self._g, int(slab), key.encode(), C.byref(v)))
        return v.value

    def set_image(self, pix):
        pix = np.ascontiguousarray(pix, dtype=np.uint8)
        assert pix.shape == (self.ny, self.nx)
        check(self._L.deff_slab_group_set_image(self._g, pix))

    def synth_image(self, seed=12345, img=0):
        check(self._L.deff_slab_group_synth_image(self._g, seed, img))

    def assemble_2phase(self, Ds, Df, CL, CR):
        check(self._L.deff_slab_group_assemble_2phase(self._g, Ds, Df, CL, CR))

    def assemble_3phase(self, Ds, Df, Dg, CL, CR, grid=None):
        """grid: the whole image's flood-fill result (NY, nx) uint32, or None."""
        g = None
        if grid is not None:
            grid = np.ascontiguousarray(grid, dtype=np.uint32)
            assert grid.shape == (self.ny, self.nx)
            g = grid.ctypes.data_as(C.c_void_p)
        check(self._L.deff_slab_group_assemble_3phase(self._g, Ds, Df, Dg, g, CL, CR))

    def init_linear(self, CL, CR):
        check(self._L.deff_slab_group_init_linear(self._g, CL, CR))

    def set_field(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.nx * self.ny
        check(self._L.deff_slab_group_set_field(self._g, x))

    def get_field(self):
        x = np.empty((self.ny, self.nx), dtype=np.float64)
        check(self._L.deff_slab_group_get_field(self._g, x))
        return x

    def sweeps(self, n, omega=OMEGA_REFERENCE):
        ms = C.c_float()
        check(self._L.deff_slab_group_sweeps(self._g, int(n), omega, C.byref(ms)))
        return ms.value

    def flux(self):
        d = C.c_double()
        MFL = np.zeros(self.ny)
        MFR = np.zeros(self.ny)
        check(self._L.deff_slab_group_flux(self._g, C.byref(d), MFL.ctypes.data_as(C.c_void_p),
                                           MFR.ctypes.data_as(C.c_void_p)))
        return d.value, MFL, MFR

    def solve(self, tol, max_iter, omega=OMEGA_REFERENCE, check_every=10000):
        res = Result()
        MFL = np.zeros(self.ny)
        MFR = np.zeros(self.ny)
        check(self._L.deff_slab_group_solve(self._g, omega, tol, int(max_iter), int(check_every), C.byref(res),
                                            MFL.ctypes.data_as(C.c_void_p), MFR.ctypes.data_as(C.c_void_p)))
        out = SolveResult()
        out.iters, out.checks = res.iters, res.checks
        out.deff_raw, out.conv, out.loop_ms = res.deff_raw, res.conv, res.loop_ms
        out.MFL, out.MFR = MFL, MFR
        return out

    def solve_cg(self, rtol=1e-10, max_iter=1_000_000, check_every=64, fluxes=True):
        """Conjugate gradients over the slabs from the current field to ||b - A x|| <= rtol ||b|| (deff_slab_group_solve_cg):
        Solver.solve_cg for an image spread over row slabs.  One slab: the bits of Solver.solve_cg."""
        return _slab_solve_cg(self._L.deff_slab_group_solve_cg, self._g, self.ny, rtol, max_iter, check_every, fluxes)


def rccl_unique_id():
    """128-byte RCCL id made on rank 0; hand it to every rank's SlabRank."""
    buf = C.create_string_buffer(128)
    check(_capi.load().deff_rccl_unique_id(buf))
    return buf.raw


class TorchDistTransport:
    """Host-staged slab transport over a torch.distributed group of CPU tensors (gloo): the halo
    blocks and the flux vectors arrive as host buffers, neighbours swap them with isend/irecv.
    For tests and for boxes without a working RCCL path between the ranks; RCCL is the fast one."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist
        self._torch, self._dist, self._group = torch, dist, group
        self.rank, self.nranks = dist.get_rank(group), dist.get_world_size(group)

    def _peer(self, r):
        return r if self._group is None else self._dist.get_global_rank(self._group, r)

    def exchange(self, send_up, recv_up, send_down, recv_down):
        t, d = self._torch, self._dist
        ops, keep = [], []
        for send, recv, peer in ((send_up, recv_up, self.rank - 1), (send_down, recv_down, self.rank + 1)):
            if send is None:
                continue
            st, rt = t.from_numpy(send.copy()), t.from_numpy(recv)
            keep += [st, rt]
            ops += [d.P2POp(d.isend, st, self._peer(peer), self._group), d.P2POp(d.irecv, rt, self._peer(peer), self._group)]
        for w in (d.batch_isend_irecv(ops) if ops else []):
            w.wait()

    def allgather(self, mine, out):
        t, d = self._torch, self._dist
        parts = [t.from_numpy(out[r]) for r in range(self.nranks)]
        d.all_gather(parts, t.from_numpy(mine.copy()), group=self._group)


class SlabRank:
    """This process's slab of one image split over `nranks` processes (one GPU each); halo
    exchange and flux all-gather go through RCCL (`unique_id`), or through `transport` (an object
    with exchange()/allgather() like TorchDistTransport) when unique_id is None.  solve() and
    sweeps() are collective."""

    def __init__(self, nx, NY, rank, nranks, unique_id=None, device=0, transport=None):
        self._L = _capi.load()
        self._s = C.c_void_p()
        self.nx, self.ny, self.rank, self.nranks = int(nx), int(NY), int(rank), int(nranks)
        if unique_id is not None:
            check(self._L.deff_slab_rank_create(int(device), self.nx, self.ny, self.rank, self.nranks, unique_id,
                                                C.byref(self._s)))
        else:
            if transport is None:
                raise ValueError("SlabRank needs an RCCL unique_id or a transport")
            self._transport, self._cb_error = transport, None

            def as_np(p, n):
                return np.ctypeslib.as_array(p, shape=(n,)) if p else None

            def xchg(_user, su, ru, sd, rd, count):
                try:
                    transport.exchange(as_np(su, count), as_np(ru, count), as_np(sd, count), as_np(rd, count))
                    return 0
                except Exception as e:                         # noqa: BLE001 -- reported through the C error path
                    self._cb_error = e
                    return 1

            def gather(_user, mine, out, count):
                try:
                    transport.allgather(as_np(mine, count), np.ctypeslib.as_array(out, shape=(self.nranks, count)))
                    return 0
                except Exception as e:                         # noqa: BLE001
                    self._cb_error = e
                    return 1

            self._cbs = (_capi.HOST_EXCHANGE_FN(xchg), _capi.HOST_ALLGATHER_FN(gather))   # keep alive
            check(self._L.deff_slab_rank_create_custom(int(device), self.nx, self.ny, self.rank, self.nranks,
                                                       self._cbs[0], self._cbs[1], None, C.byref(self._s)))
        self._ctx = C.c_void_p()
        check(self._L.deff_slab_rank_context(self._s, C.byref(self._ctx)))

    def close(self):
        if self._s:
            self._L.deff_slab_rank_destroy(self._s)
            self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _pair(self, fn):
        a, b = C.c_int(), C.c_int()
        check(fn(self._s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def layout(self):
        """(first owned row, owned rows)"""
        return self._pair(self._L.deff_slab_rank_layout)

    def window(self):
        """(first row held incl. halo, rows held): the slice of the image set_image() takes"""
        return self._pair(self._L.deff_slab_rank_window)

    def set_tuning(self, key, value):
        check(self._L.deff_slab_rank_set_tuning(self._s, key.encode(), int(value)))

    def set_image(self, pix_full):
        a, n = self.window()
        win = np.ascontiguousarray(pix_full[a:a + n], dtype=np.uint8)
        check(self._L.deff_slab_rank_set_image_window(self._s, win))

    def synth_image(self, seed=12345, img=0):
        check(self._L.deff_slab_rank_synth_image(self._s, seed, img))

    def assemble_2phase(self, Ds, Df, CL, CR):
        check(self._L.deff_assemble_2phase(self._ctx, Ds, Df, CL, CR))

    def assemble_3phase(self, Ds, Df, Dg, CL, CR, grid_full=None):
        """grid_full: the whole image's flood-fill result (NY, nx); this rank passes its window of it."""
        g = None
        if grid_full is not None:
            a, n = self.window()
            win = np.ascontiguousarray(grid_full[a:a + n], dtype=np.uint32)
            g = win.ctypes.data_as(C.c_void_p)
        check(self._L.deff_slab_rank_assemble_3phase(self._s, Ds, Df, Dg, g, CL, CR))

    def init_linear(self, CL, CR):
        check(self._L.deff_init_linear(self._ctx, CL, CR))

    def get_field(self):
        _, own = self.layout()
        x = np.empty((own, self.nx), dtype=np.float64)
        check(self._L.deff_slab_rank_get_field(self._s, x))
        return x

    def sweeps(self, n, omega=OMEGA_REFERENCE):
        ms = C.c_float()
        check(self._L.deff_slab_rank_sweeps(self._s, int(n), omega, C.byref(ms)))
        return ms.value

    def solve(self, tol, max_iter, omega=OMEGA_REFERENCE, check_every=10000):
        res = Result()
        MFL = np.zeros(self.ny)
        MFR = np.zeros(self.ny)
        check(self._L.deff_slab_rank_solve(self._s, omega, tol, int(max_iter), int(check_every), C.byref(res),
                                           MFL.ctypes.data_as(C.c_void_p), MFR.ctypes.data_as(C.c_void_p)))
        out = SolveResult()
        out.iters, out.checks = res.iters, res.checks
        out.deff_raw, out.conv, out.loop_ms = res.deff_raw, res.conv, res.loop_ms
        out.MFL, out.MFR = MFL, MFR
        return out

    def solve_cg(self, rtol=1e-10, max_iter=1_000_000, check_every=64, fluxes=True):
        """SlabGroup.solve_cg, collective over the ranks (deff_slab_rank_solve_cg): every rank gets the same CGResult."""
        return _slab_solve_cg(self._L.deff_slab_rank_solve_cg, self._s, self.ny, rtol, max_iter, check_every, fluxes)

    def plan_value(self, key):
        v = C.c_int()
        check(self._L.deff_get_plan(self._ctx, key.encode(), C.byref(v)))
        return v.value


def load_jpeg_gray(path):
    """Grayscale JPEG -> uint8 (H, W), decoded like the reference's stbi_load(..., 1)."""
    L = _capi.load()
    p = C.c_void_p()
    w, h, n = C.c_int(), C.c_int(), C.c_int()
    check(L.deff_load_jpeg_gray(str(path).encode(), C.byref(p), C.byref(w), C.byref(h), C.byref(n)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(h.value, w.value)).copy()
    finally:
        L.deff_free(p)


def flood_fill(grid):
    """FloodFill (Deff2D.cuh:557-713): grid (ny, nx) with 1 = solid -> (grid with unreachable
    pore cells = 2, PathFlag).  Host function of the library; needs no GPU."""
    g = np.array(grid, dtype=np.uint32, order="C", copy=True)
    ny, nx = g.shape
    flag = C.c_int()
    check(_capi.load().deff_flood_fill(g, nx, ny, C.byref(flag)))
    return g, bool(flag.value)


__all__ = ["Solver", "SlabGroup", "SlabRank", "rccl_unique_id", "flood_fill", "load_jpeg_gray", "SolveResult", "DeffError", "OMEGA_REFERENCE"]
