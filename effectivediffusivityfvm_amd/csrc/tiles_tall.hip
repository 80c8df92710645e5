// tiles_tall.hip -- the tall 16-wave workgroup tiles (tile_kernels.hpp): k_sweep_wgres<.., TALL> and k_sweep_wgage, instantiated
// here only.
#include "tile_kernels.hpp"

// Tall tiles: 16 waves, the rows of ages 0..3 summing to 4R, matrix rows looked up in every sweep (4 waves per SIMD).  Rows dealt
// by age run k_sweep_wgage, equal rows k_sweep_wgres<.., TALL>.  Unguarded with and without the link-symmetric short-cut; the
// guarded kernel branches on every link anyway and exists with equal rows only.
template <int A, int B, int C, int D, bool F, bool G, bool SYM> static constexpr ResidentKernel tall_instance()
{
    if constexpr (A == D) return k_sweep_wgres<8, A, F, G, true, SYM>;
    else return k_sweep_wgage<8, A, B, C, D, F, G, SYM>;
}
template <int R, int A = R, int B = R, int C = R, int D = R> static constexpr auto tall()
{
    static_assert(A + B + C + D == 4 * R, "rows dealt by age keep the tile of 16 R rows");
    const auto unguarded = by_flags([](auto f, auto s) {
        constexpr bool F = decltype(f)::value, S = decltype(s)::value;
        return TileKernel{WGL_WAVES, 8, {A, B, C, D}, R, F, false, S, tall_instance<A, B, C, D, F, false, S>()};
    });
    if constexpr (A != D) return unguarded;
    else return cat(unguarded, by_flag([](auto f) {
        constexpr bool F = decltype(f)::value;
        return TileKernel{WGL_WAVES, 8, {R, R, R, R}, R, F, true, false, tall_instance<R, R, R, R, F, true, false>()};
    }));
}

const std::array<TileKernel, 98> TILES_TALL = cat(
    // (tall R = 16 -- 256-row tiles, images up to ~2600^2 -- spills inside the sweep loop: 9.9 us per sweep, slower than streaming)
    tall<4>(), tall<5>(), tall<6>(), tall<7>(), tall<8>(), tall<9>(), tall<10>(), tall<11>(), tall<12>(), tall<13>(), tall<14>(),
    // Rows by age for the tall tiles of R rows per wave: the 4R rows of a SIMD's four waves, oldest first.  Measured, not derived
    // (profiles/r04_tall_rows_by_age_kbench.log: four candidate sets per R, one process, against equal rows): what wins gives the
    // youngest wave about half its share and keeps the three older ones level; bodies of 9 and more rows spill, which is why R = 7
    // stops at 8 rows, R = 9 deals one row only, and R = 13 found no set that beats equal rows -- four equal bodies in this kernel
    // run 3-4 % behind the one-body kernel, which is what every set has to earn first (14 x 4 has nothing to deal).  Unguarded
    // systems, link-symmetric (7 lookups per row) or not (10: the 3-phase assembly with impermeable solid), both arithmetics.
    tall<5, 6, 6, 5, 3>(), tall<6, 8, 8, 5, 3>(), tall<7, 8, 8, 8, 4>(), tall<8, 9, 9, 9, 5>(), tall<9, 10, 9, 9, 8>(),
    tall<10, 12, 12, 10, 6>(), tall<11, 13, 13, 11, 7>(), tall<12, 13, 13, 13, 9>());
