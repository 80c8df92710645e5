// kernels_cg_stream.hpp -- the slot life cycle of deff_solve_cg_stream (api_cg.hip, DESIGN.md section 9, "Stream"): what
// happens to the slots of a stack that an image ENTERS or LEAVES while the others go on iterating.  The iteration itself is
// that of kernels_cg.hpp / kernels_cg_image.hpp, untouched: those kernels skip every image whose CgScal::done is not 0, so a
// slot is theirs between its entry check (done = 0) and its stop, and belongs to the kernels below otherwise.
//
// Every kernel here takes a device LIST of slots and launches work for the listed slots only; nothing of an unlisted slot
// is read or written (k_cg_resid rewrites r and x of every image of the stack, which is safe only when all of them stand
// still).  One launch serves any number of slots, so a host check costs the same few launches however many images retire
// or enter in it.
//   k_cgs_enter       pixels (staged by one H2D copy) -> the slot's pixels, 16-bit codes, wall diffusivities, linear guess:
//                     the arithmetic of k_phase_codes, k_wall_D_2phase and k_init_linear (kernels_setup.hpp)
//   k_cgs_admissible  k_cg_admissible's rule (cg_cell_bad) on the listed slots
//   k_cgs_resid       k_cg_resid of the listed slots: the same work items (cg_item) and row walk (cg_resid_rows), partials per image
//   k_cgs_check       k_cg_check of the listed slots (cg_check_step); the restart allowance of mode 1 is the slot's own count of rounds
//   k_cgs_flux        the wall fluxes of the listed slots and their sums {Q1, Q2} (k_wall_flux, k_flux_sum)
// Partial sums are stored by LIST POSITION (cg_item / cg_image_sum index them by the launch's image number), images by slot.
//
// Determinism: an image's items, their wave sums and the order in which its workgroup adds them are those of a one-image
// context (the geometry depends on (nx, ny) alone), so entry (mode 0) and true-residual round (mode 1) give its bits.
#pragma once
#include "kernels_cg.hpp"
#include "kernels_setup.hpp"

namespace deff {

// r = b - A x of the listed slots; g.nimg = the number of listed slots.  cg_resid_rows on the slot's window.
__global__ __launch_bounds__(256) void k_cgs_resid(const double *__restrict__ tab_g, int nrows, const uint16_t *__restrict__ code,
                                                   double *__restrict__ x, double *__restrict__ r, CgGeom g,
                                                   const int *__restrict__ list, double *__restrict__ partial)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CgItem it;
    if (!cg_item(g, wave, lane, it)) return;
    const CgWin w{(size_t)list[it.img] * g.ny * g.nx, 0, g.ny};  // the cells of the listed slot; it.idx stays the list's
    double s1, s2, s3;
    cg_resid_rows(tab, code, x, r, w, g.nx, it.col, it.l0, it.l1, cg_halo_col(g.nx, it.col, lane), s1, s2, s3);
    if (lane == 63) cg_store3(partial, it.idx, s1, s2, s3);
}

// after k_cgs_resid, one workgroup per listed slot.  mode 0: the slot's image starts (its rounds count from 0);  mode 1: the
// true residual of a stopped image stands, or -- it misses rtol, the slot has restart rounds and iterations left -- the image
// goes on from the true r (done = 0: the iteration kernels take it up again with the next launch).
__global__ __launch_bounds__(CG_FIN) void k_cgs_check(const double *__restrict__ part, unsigned per_img, CgScal *__restrict__ sc,
                                                      const int *__restrict__ list, int *__restrict__ rounds, double tol2,
                                                      long long max_iter, int mode, int max_rounds)
{
    __shared__ double ws[4];
    const int slot = list[blockIdx.x];
    const double *pp = part + (size_t)blockIdx.x * per_img * 3;
    const double rr = cg_image_sum(pp, per_img, 3, 0, ws);
    const double rz = cg_image_sum(pp, per_img, 3, 1, ws);
    const double bb = cg_image_sum(pp, per_img, 3, 2, ws);
    if (threadIdx.x != 0) return;
    const bool again = cg_check_step(sc[slot], rr, rz, bb, tol2, max_iter, mode, rounds[slot] < max_rounds);
    if (mode == 0) rounds[slot] = 0;
    else if (again) rounds[slot] += 1;
}

// Entry of the listed slots: image `blockIdx.y` of the staging buffer becomes the image of slot list[blockIdx.y].
// (DCF / DCS: fluid / solid diffusivity; `contracted` as in k_init_linear.)
__global__ __launch_bounds__(256) void k_cgs_enter(const uint8_t *__restrict__ stage, const int *__restrict__ list, int W, int H,
                                                   int ampX, int ampY, int nx, int nxt, int ny, double DCF, double DCS, double CL,
                                                   double CR, int contracted, uint8_t *__restrict__ pix,
                                                   uint16_t *__restrict__ code, double *__restrict__ Dl, double *__restrict__ Dr,
                                                   double *__restrict__ x)
{
    const int slot = list[blockIdx.y];
    const size_t npix = (size_t)W * H, n_img = (size_t)nx * ny;
    const uint8_t *src = stage + (size_t)blockIdx.y * npix;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t q = t0; q < npix; q += stride) pix[(size_t)slot * npix + q] = src[q];
    for (size_t q = t0; q < (size_t)ny; q += stride) {                                          // k_wall_D_2phase
        const int i = (int)q;
        Dl[(size_t)slot * ny + i] = (cell_pixel(src, W, ampX, ampY, ny, i, 0) < 150) ? DCF : DCS;
        Dr[(size_t)slot * ny + i] = (cell_pixel(src, W, ampX, ampY, ny, i, nxt - 1) < 150) ? DCF : DCS;
    }
    uint16_t *cd = code + (size_t)slot * n_img;
    double *xs = x + (size_t)slot * n_img;
    for (size_t p = t0; p < n_img; p += stride) {
        const int i = (int)(p / nx), j = (int)(p % nx);
        if (j >= nxt) { cd[p] = 0; xs[p] = 0.0; continue; }
        const int jw = j > 0 ? j - 1 : j, je = j < nxt - 1 ? j + 1 : j;                         // k_phase_codes
        const int is = i < ny - 1 ? i + 1 : i, in = i > 0 ? i - 1 : i;
        unsigned c = (cell_pixel(src, W, ampX, ampY, ny, i, j) >= 150) ? 1u : 0u;
        c |= (cell_pixel(src, W, ampX, ampY, ny, i, jw) >= 150) ? 2u : 0u;
        c |= (cell_pixel(src, W, ampX, ampY, ny, i, je) >= 150) ? 4u : 0u;
        c |= (cell_pixel(src, W, ampX, ampY, ny, is, j) >= 150) ? 8u : 0u;
        c |= (cell_pixel(src, W, ampX, ampY, ny, in, j) >= 150) ? 16u : 0u;
        const unsigned cls = (unsigned)(pos_class(i, ny) * 3 + pos_class(j, nxt));
        cd[p] = (uint16_t)((1u + cls * 32u + c) * 8u);
        xs[p] = contracted ? __builtin_fma((double)j / nxt, (CR - CL), CL) : (double)j / nxt * (CR - CL) + CL;   // k_init_linear
    }
}

// k_cg_admissible's rule on the listed slots (blockIdx.y = position in the list)
__global__ __launch_bounds__(256) void k_cgs_admissible(const double *__restrict__ tab_g, int nrows,
                                                        const uint16_t *__restrict__ code, int nx, int ny,
                                                        const int *__restrict__ list, unsigned *flag)
{
    __shared__ double tab[CG_DOUBLES];
    cg_load_tab(tab, tab_g, nrows);
    const size_t n = (size_t)nx * ny;
    const uint16_t *cd = code + (size_t)list[blockIdx.y] * n;
    bool bad = false;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        if (cg_v<CG_INV>(tab, cd[p]) == 0.0) continue;
        const int li = (int)(p / nx), j = (int)(p - (size_t)li * nx);
        bad |= cg_cell_bad(tab, cd, p, j, nx, li > 0 ? CG_NEIGHBOUR : CG_WALL, li + 1 < ny ? CG_NEIGHBOUR : CG_WALL);
    }
    if (bad) atomicOr(flag, 1u);
}

// Wall fluxes of the listed slots' rows (k_wall_flux's expressions, into the stack's mf) and their sums q[slot] = {Q1, Q2}:
// in row order by one lane, which is deff_flux's order on the host and on the device, or -- `tree`, flux_reduce 2 --
// k_flux_sum<true>'s butterfly.  One workgroup per listed slot.
__global__ __launch_bounds__(256) void k_cgs_flux(const double *__restrict__ x, const double *__restrict__ Dl,
                                                  const double *__restrict__ Dr, int nx, int nxt, int ny, int rows, double dx,
                                                  double CL, double CR, const int *__restrict__ list, int tree,
                                                  double *mf, double *__restrict__ q)
{
    const int slot = list[blockIdx.x];
    for (int j = threadIdx.x; j < ny; j += 256) {
        const size_t i = (size_t)slot * ny + j;
        mf[i] = Dl[i] * (x[i * nx] - CL) / (dx / 2.0);
        mf[rows + i] = Dr[i] * (CR - x[i * nx + nxt - 1]) / (dx / 2.0);
    }
    __syncthreads();                                             // the workgroup's own stores, read back below
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const double *L = mf + (size_t)slot * ny, *R = mf + rows + (size_t)slot * ny;
    double q1 = 0, q2 = 0;
    if (tree) {
        for (int j = lane; j < ny; j += 64) { q1 += L[j]; q2 += R[j]; }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            q1 += __shfl_xor(q1, off, 64);
            q2 += __shfl_xor(q2, off, 64);
        }
    } else {
        if (lane != 0) return;
        for (int j = 0; j < ny; ++j) { q1 += L[j]; q2 += R[j]; }
    }
    if (lane == 0) { q[2 * slot] = q1; q[2 * slot + 1] = q2; }
}

}  // namespace deff
