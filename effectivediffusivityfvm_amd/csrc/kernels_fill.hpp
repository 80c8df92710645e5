// kernels_fill.hpp -- the flood fill of the pore space on the device (gfx950) and what the native 3-phase assembly makes of
// it: row codes, wall diffusivities, the Grid in the reference's encoding.  flood_fill.hpp is the specification; the step of
// one bitmap word is fill_step.hpp (shared with the host test), the row numbering row_index3.hpp.
//
// Bitmaps in global memory: open[rows][nw] and reach[rows][nw], nw = words of 64 columns per row, image k of a stack = rows
// [k ny, (k + 1) ny).  Two forms:
//   k_fill_image   one workgroup per image: bitmaps built from the pixels straight into LDS (a wave's ballot of the pixel test
//                  is a word), rounds to the fixed point with one barrier each, one launch;
//   k_fill_tiles   images too large for that: row tiles of the whole width, a one-row halo of reach above and below read from
//                  global memory (periodic between the image's first and last row).  A launch brings every tile to its LOCAL
//                  fixed point; a tile that grew writes its rows back and ORs into its image's `changed` word.  The host
//                  enqueues launches until a launch changed nothing.
// No workgroup waits for another: within a launch a tile may or may not see what its neighbour writes in the same launch,
// and either is right, because bits are only ever set and every set bit is a reached cell.  Every loop ends by itself (a
// round without a change) and is bounded besides (fill_round_cap).  Vector stores and atomics only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fill_step.hpp"
#include "kernels_setup.hpp"
#include "row_index3.hpp"

namespace deff {

constexpr int FILL_SMALL_WORDS = 1024, FILL_SMALL_THREADS = 256;    // 16 KiB of LDS: up to ten images per compute unit
constexpr int FILL_LARGE_WORDS = 8192, FILL_LARGE_THREADS = 1024;   // 128 KiB of LDS
constexpr int FILL_STATUS = 4;                                      // ints per image: PathFlag, hit the round cap, rounds, -

__device__ __forceinline__ bool fill_open_cell(const uint8_t *pix, int W, int ampX, int ampY, int ny, int nxt, int i, int col)
{
    return col < nxt && cell_pixel(pix, W, ampX, ampY, ny, i, col) <= 200;
}

// Rounds over a tile of `rows` x nw words in LDS until nothing changes.  m: open words, r: reach words (updated in place: a
// word is written by the one thread that owns it, read by its neighbours' owners whenever), above0 / belowL: the nw reach
// words above the tile's first row and below its last.  Returns the rounds taken; *capped when the last one still changed.
template <int NT>
__device__ __forceinline__ long long fill_rounds(const uint64_t *m, uint64_t *r, const uint64_t *above0, const uint64_t *belowL,
                                                 int rows, int nw, long long cap, bool *grew, bool *capped)
{
    const int nwords = rows * nw;
    long long round = 0;
    int more = 1;
    bool any = false;
    for (; more && round < cap; ++round) {
        int ch = 0;
        for (int k = threadIdx.x; k < nwords; k += NT) {
            const uint64_t mm = m[k], own = r[k];
            if (own == mm) continue;                                 // closed, or reached all over
            const int i = k / nw, w = k - i * nw;
            const uint64_t ab = i == 0 ? above0[w] : r[k - nw];
            const uint64_t be = i == rows - 1 ? belowL[w] : r[k + nw];
            const uint64_t le = w ? r[k - 1] : 0ull, ri = w < nw - 1 ? r[k + 1] : 0ull;
            const uint64_t nv = fill_word(mm, own, ab, be, le, ri);
            if (nv != own) { r[k] = nv; ch = 1; }
        }
        more = __syncthreads_or(ch);
        any |= more != 0;
    }
    *grew = any;
    *capped = more != 0;
    return round;
}

// PathFlag of one image by one workgroup: a reached cell in the last column, or the quirk
template <int NT>
__device__ __forceinline__ int fill_path_of(const uint64_t *reach_rows, int ny, int nw, int nxt, bool quirk)
{
    int hit = 0;
    const int w = (nxt - 1) >> 6, b = (nxt - 1) & 63;
    for (int i = threadIdx.x; i < ny; i += NT) hit |= (int)((reach_rows[(size_t)i * nw + w] >> b) & 1ull);
    return (__syncthreads_or(hit) || quirk) ? 1 : 0;
}

// Form 1.  grid = images, CAP >= ny * nw.
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void k_fill_image(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nxt, int ny,
                                                   int nw, long long cap, uint64_t *__restrict__ open_g,
                                                   uint64_t *__restrict__ reach_g, int *__restrict__ status)
{
    __shared__ uint64_t m[CAP], r[CAP];
    const int img = blockIdx.x, nwords = ny * nw, lane = threadIdx.x & 63;
    const bool quirk = cell_pixel(pix, W, ampX, ampY, ny, img * ny, 0) > 200;
    for (int k = threadIdx.x >> 6; k < nwords; k += NT / 64) {
        const int i = k / nw, w = k - i * nw;
        const uint64_t word = __ballot(fill_open_cell(pix, W, ampX, ampY, ny, nxt, img * ny + i, w * 64 + lane));
        if (lane == 0) { m[k] = word; r[k] = word & fill_seed_mask(w, nxt, quirk); }
    }
    __syncthreads();
    bool grew, capped;
    const long long rounds = fill_rounds<NT>(m, r, r + (size_t)(ny - 1) * nw, r, ny, nw, cap, &grew, &capped);
    uint64_t *og = open_g + (size_t)img * nwords, *rg = reach_g + (size_t)img * nwords;
    for (int k = threadIdx.x; k < nwords; k += NT) { og[k] = m[k]; rg[k] = r[k]; }
    const int path = fill_path_of<NT>(r, ny, nw, nxt, quirk);
    if (threadIdx.x == 0) {
        int *st = status + img * FILL_STATUS;
        st[0] = path; st[1] = capped ? 1 : 0; st[2] = (int)(rounds > 0x7fffffff ? 0x7fffffff : rounds); st[3] = 0;
    }
}

// Form 2, first launch: open words and seeds of the whole stack, one wave per word; the status is cleared.
__global__ __launch_bounds__(256) void k_fill_open(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nxt, int ny,
                                                   int nw, int nimg, uint64_t *__restrict__ open_g,
                                                   uint64_t *__restrict__ reach_g, int *__restrict__ status)
{
    const size_t total = (size_t)nimg * ny * nw;
    const int lane = threadIdx.x & 63;
    for (size_t k = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < total; k += (size_t)gridDim.x * 4) {
        const int row = (int)(k / nw), w = (int)(k - (size_t)row * nw), img = row / ny;
        const bool quirk = cell_pixel(pix, W, ampX, ampY, ny, img * ny, 0) > 200;
        const uint64_t word = __ballot(fill_open_cell(pix, W, ampX, ampY, ny, nxt, row, w * 64 + lane));
        if (lane == 0) { open_g[k] = word; reach_g[k] = word & fill_seed_mask(w, nxt, quirk); }
    }
    for (int k = blockIdx.x * 256 + threadIdx.x; k < nimg * FILL_STATUS; k += gridDim.x * 256) status[k] = 0;
}

// Form 2, every launch.  grid = images x ntiles workgroups; tile t = rows [t tr, min(ny, (t + 1) tr)) of its image, (tr + 2) nw <= CAP.
// prev: the images' `changed` words of the launch before (an image that was at its fixed point then is at it now), or null.
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void k_fill_tiles(const uint64_t *__restrict__ open_g, uint64_t *reach_g, int nxt, int ny,
                                                   int nw, int tr, int ntiles, long long cap, const unsigned *__restrict__ prev,
                                                   unsigned *__restrict__ changed, int *__restrict__ status)
{
    __shared__ uint64_t m[CAP], r[CAP];
    const int img = blockIdx.x / ntiles;
    if (prev && prev[img] == 0) return;
    const int r0 = (blockIdx.x - img * ntiles) * tr, rows = min(tr, ny - r0), nwords = rows * nw;
    if (rows <= 0) return;
    const size_t base = (size_t)img * ny * nw;
    const uint64_t *og = open_g + base + (size_t)r0 * nw;
    uint64_t *rg = reach_g + base + (size_t)r0 * nw;
    // LDS rows: 0 = the row above the tile, 1 .. rows = the tile, rows + 1 = the row below
    const uint64_t *ha = reach_g + base + (size_t)(r0 == 0 ? ny - 1 : r0 - 1) * nw;
    const uint64_t *hb = reach_g + base + (size_t)(r0 + rows == ny ? 0 : r0 + rows) * nw;
    for (int k = threadIdx.x; k < nwords; k += NT) { m[k] = og[k]; r[nw + k] = rg[k]; }
    for (int w = threadIdx.x; w < nw; w += NT) {
        r[w] = ha[w];                                                // (may be a neighbour's store of this launch: either value is right)
        r[(size_t)(rows + 1) * nw + w] = hb[w];
    }
    __syncthreads();
    bool grew, capped;
    const long long rounds = fill_rounds<NT>(m, r + nw, r, r + (size_t)(rows + 1) * nw, rows, nw, cap, &grew, &capped);
    if (!grew) return;
    for (int k = threadIdx.x; k < nwords; k += NT) rg[k] = r[nw + k];
    if (threadIdx.x == 0) {
        atomicOr(&changed[img], 1u);
        int *st = status + img * FILL_STATUS;
        if (capped) atomicOr(&st[1], 1);
        atomicMax(&st[2], (int)(rounds > 0x7fffffff ? 0x7fffffff : rounds));
    }
}

// Form 2, last launch: PathFlag per image.  grid = images.
__global__ __launch_bounds__(256) void k_fill_path(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nxt, int ny,
                                                   int nw, const uint64_t *__restrict__ reach_g, int *__restrict__ status)
{
    const int img = blockIdx.x;
    const bool quirk = cell_pixel(pix, W, ampX, ampY, ny, img * ny, 0) > 200;
    const int path = fill_path_of<256>(reach_g + (size_t)img * ny * nw, ny, nw, nxt, quirk);
    if (threadIdx.x == 0) status[img * FILL_STATUS] = path;
}

__device__ __forceinline__ bool fill_reached(const uint64_t *__restrict__ reach_g, int nw, int i, int j)
{
    return (reach_g[(size_t)i * nw + (j >> 6)] >> (j & 63)) & 1ull;
}

// The fill in the reference's encoding (FloodFill's Grid): 1 solid, 2 not reached, 0 reached; pad column 0.
static __global__ void k_fill_grid(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nx, int nxt, int ny, int rows,
                                   const uint64_t *__restrict__ reach_g, int nw, unsigned int *__restrict__ Grid)
{
    const size_t n = (size_t)nx * rows;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(p / nx), j = (int)(p % nx);
        if (j >= nxt) { Grid[p] = 0; continue; }
        Grid[p] = cell_pixel(pix, W, ampX, ampY, ny, i, j) > 200 ? 1u : (fill_reached(reach_g, nw, i, j) ? 0u : 2u);
    }
}

// Row codes of the native 3-phase system (row_index3.hpp): identity row where Grid would be 1 or 2, else the row of the
// cell's own phase and its neighbours' pixel classes.  Neighbours outside the image read the clamped cell; the position
// class has no link to them.  used[16]: one bit per table row that some cell got (ORed in; the caller clears it) -- the host
// keeps the rows no cell uses out of the table's singular-row test (api_fill.hip).
static __global__ void k_phase_codes3(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nx, int nxt, int ny,
                                      int rows, const uint64_t *__restrict__ reach_g, int nw, uint16_t *__restrict__ code,
                                      unsigned *__restrict__ used)
{
    __shared__ unsigned su[16];
    if (threadIdx.x < 16) su[threadIdx.x] = 0;
    __syncthreads();
    const size_t n = (size_t)nx * rows;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(p / nx), j = (int)(p % nx);
        if (j >= nxt) { code[p] = 0; continue; }
        const unsigned v = cell_pixel(pix, W, ampX, ampY, ny, i, j);
        if (v > 200 || !fill_reached(reach_g, nw, i, j)) { code[p] = (uint16_t)(NATIVE3_IDENTITY * 8); continue; }
        const int li = i % ny;
        const int jw = j > 0 ? j - 1 : j, je = j < nxt - 1 ? j + 1 : j;
        const int is = li < ny - 1 ? i + 1 : i, in = li > 0 ? i - 1 : i;
        const int row = native3_row(pos_class(li, ny), pos_class(j, nxt), v < 50 ? 1 : 0,
                                    native3_pixel_class(cell_pixel(pix, W, ampX, ampY, ny, i, jw)),
                                    native3_pixel_class(cell_pixel(pix, W, ampX, ampY, ny, i, je)),
                                    native3_pixel_class(cell_pixel(pix, W, ampX, ampY, ny, is, j)),
                                    native3_pixel_class(cell_pixel(pix, W, ampX, ampY, ny, in, j)));
        code[p] = (uint16_t)(row * 8);
        if (!(su[row >> 5] & (1u << (row & 31)))) atomicOr(&su[row >> 5], 1u << (row & 31));
    }
    __syncthreads();
    if (threadIdx.x < 16 && su[threadIdx.x]) atomicOr(&used[threadIdx.x], su[threadIdx.x]);
}

// Diffusivity of the first and last cell of every row (cuh:1256-1257 read D there), three pixel classes.
static __global__ void k_wall_D_3phase(const uint8_t *__restrict__ pix, int W, int ampX, int ampY, int nxt, int ny, int rows,
                                       double DCF, double DCS, double DCG, double *__restrict__ Dl, double *__restrict__ Dr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint8_t a = cell_pixel(pix, W, ampX, ampY, ny, i, 0), b = cell_pixel(pix, W, ampX, ampY, ny, i, nxt - 1);
    Dl[i] = (a > 200) ? DCS : (a < 50 ? DCG : DCF);
    Dr[i] = (b > 200) ? DCS : (b < 50 ? DCG : DCF);
}

}  // namespace deff
