// fill_step.hpp -- the flood fill on bitmaps: what one 64-column word does in one round, the seeds and the bounds.
// Plain C++ that also compiles for the device (FILL_HD), so that tests/cpp/fill_bits.cpp runs the very text the kernels
// of kernels_fill.hpp run.  flood_fill.hpp is the specification (the reference's FloodFill, cuh:557-713).
//
// Bitmaps: one `open` word (cell is not solid) and one `reach` word (cell was visited) per 64 columns of a row, bit b of
// word w = column 64 w + b; columns past the mesh are closed.  reach is a subset of open, always, and only ever grows.
//
// A round of a word: the seeds s are what it has reached already, what the rows above and below have reached in the same
// columns, and the neighbouring words' edge bits; a seed then fills its whole run of open bits.  Upwards a run costs one
// add: m + s carries from the seed to the end of its run, so (m + s) ^ m has exactly the bits the carry went through
// (and the closed bit that stopped it, which & m drops; s is a subset of m, so a carry never meets a seed outside a run).
// Downwards it is the same on the bit-reversed words.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FILL_HD __host__ __device__ inline
#else
#define FILL_HD inline
#endif

namespace deff {

FILL_HD uint64_t fill_rev64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brevll(v);
#else
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    v = ((v >> 8) & 0x00FF00FF00FF00FFull) | ((v & 0x00FF00FF00FF00FFull) << 8);
    v = ((v >> 16) & 0x0000FFFF0000FFFFull) | ((v & 0x0000FFFF0000FFFFull) << 16);
    return (v >> 32) | (v << 32);
#endif
}

// every open bit of m that lies in a run with a bit of s (s is masked to m here)
FILL_HD uint64_t fill_runs(uint64_t m, uint64_t s)
{
    s &= m;
    const uint64_t up = (((m + s) ^ m) | s) & m;
    const uint64_t mr = fill_rev64(m), sr = fill_rev64(s);
    const uint64_t dn = (((mr + sr) ^ mr) | sr) & mr;
    return up | fill_rev64(dn);
}

// One round of one word: m its open bits, own / above / below the reach of the word itself and of the same columns one row
// up and down (for the first and last row of an image: the last and first, the fill is periodic there), left / right the
// reach of the neighbouring words of the row (0 at the image's first and last word: not periodic between columns).
FILL_HD uint64_t fill_word(uint64_t m, uint64_t own, uint64_t above, uint64_t below, uint64_t left, uint64_t right)
{
    return fill_runs(m, own | above | below | (left >> 63) | (right << 63));
}

// The seed columns of word w of a row as a mask (to be ANDed with the word's open bits): column 0, and when the image's
// top-left cell is solid the last two columns as well -- the reference's quirk (cuh:601): every last-column cell is then
// seeded, solid or not; a solid seed spreads to its non-solid neighbours (the last column's, which are seeds themselves,
// and the one to its west) and stays solid.
FILL_HD uint64_t fill_seed_mask(int w, int nxt, bool top_left_solid)
{
    uint64_t s = w == 0 ? 1ull : 0ull;
    if (top_left_solid)
        for (int col = nxt - 2 > 0 ? nxt - 2 : 0; col < nxt; ++col)
            if ((col >> 6) == w) s |= 1ull << (col & 63);
    return s;
}

// columns of word w that are inside a mesh of nxt columns
FILL_HD uint64_t fill_mesh_mask(int w, int nxt)
{
    const int left = nxt - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

FILL_HD int fill_words(int nxt) { return (nxt + 63) >> 6; }

// Rounds a workgroup may take over `rows` rows of nxt columns.  Every round but the last sets at least one bit and there
// are rows * nxt of them, so a fill that is still changing after this many rounds does not exist: the bound only makes the
// loop's end independent of the data.
FILL_HD long long fill_round_cap(int rows, int nxt) { return (long long)rows * nxt + 2; }

// Launches the tiled form is given for an image of ny x nxt cells before the image goes to the host fill (which is linear
// in the cells; a launch costs what ~16 Ki cells of it cost).  Not a bound on what a fill may need: a path that winds through
// every seam many times gets there, and is then filled on the host.
FILL_HD int fill_launch_cap(int ny, int nxt)
{
    const long long c = 64 + (long long)ny * nxt / 16384;
    return c > 4096 ? 4096 : (int)c;
}

}  // namespace deff
