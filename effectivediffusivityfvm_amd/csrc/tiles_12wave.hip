// tiles_12wave.hip -- the link-symmetric 12-wave workgroup tiles (tile_kernels.hpp): k_sweep_wgsym and k_sweep_wgsage,
// instantiated here only.
#include "tile_kernels.hpp"

// Link-symmetric 12-wave tiles, the rows of ages 0..2 (3 waves per SIMD): k_sweep_wgsym for equal rows, k_sweep_wgsage.
template <int T, int A, int B, int C, bool F> static constexpr ResidentKernel sym_instance()
{
    if constexpr (A == C) return k_sweep_wgsym<T, A, F>;
    else return k_sweep_wgsage<T, A, B, C, F>;
}
template <int T, int A, int B, int C> static constexpr auto sym()
{
    return by_flag([](auto f) {
        constexpr bool F = decltype(f)::value;
        return TileKernel{WGS_WAVES, T, {A, B, C, 0}, A, F, false, true, sym_instance<T, A, B, C, F>()};
    });
}

const std::array<TileKernel, 18> TILES_12WAVE = cat(
    // For T = 8 also the shapes that give the younger waves a row less (k_sweep_wgsage): 5 / 5 / 4 is a 56-row tile
    // that sweeps ~9 % faster than 5 / 5 / 5 and owns 40 rows instead of 44 -- one 1024^2 image: 234 tiles instead of 216, 853 ->
    // 901 G; 4 / 4 / 3 and 5 / 4 / 4 likewise (704^2 ... 992^2: +6 ... 11 %, profiles/r04_sym_shapes_kbench.log).  The tests
    // address T = 8's list by its 1-based position (tuning "tb_sym_shape").
    // (R = 6 -- 72-row tiles, images up to ~1230^2 -- needs 168 VGPRs + ~100 B of scratch, which lands in the halo exchange: 1152^2
    // 652 G against 704 G on tall tiles: not instantiated; R = 3 -- 36-row tiles -- is no faster than 8 waves x 4 rows, see
    // plan_blocked_pass, api_sweep.hip)
    sym<8, 4, 4, 3>(), sym<8, 4, 4, 4>(), sym<8, 5, 4, 4>(), sym<8, 5, 5, 4>(), sym<8, 5, 5, 5>(),
    sym<6, 4, 4, 4>(), sym<6, 5, 5, 5>(), sym<4, 4, 4, 4>(), sym<4, 5, 5, 5>());
