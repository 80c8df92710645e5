// tiles_8wave.hip -- the 8-wave workgroup tiles (tile_kernels.hpp): k_sweep_wgtile and k_sweep_wgres, instantiated here only.
#include "tile_kernels.hpp"

// 8 waves x R rows, matrix rows in registers (2 waves per SIMD): resident (k_sweep_wgres) or one launch per pass
// (k_sweep_wgtile).  R = 8 needs 256 VGPRs + 148 B of scratch per lane and ran 40 % SLOWER than R = 6: the spills sit in the
// sweep loop.
template <int T, int... R> static constexpr auto tiles8()
{
    return cat(by_flags([](auto f, auto g) {
        constexpr bool F = decltype(f)::value, G = decltype(g)::value;
        return TileKernel{WGT_WAVES, T, {R, R, 0, 0}, R, F, G, false, k_sweep_wgres<T, R, F, G>, k_sweep_wgtile<T, R, F, G>};
    })...);
}

const std::array<TileKernel, 24> TILES_8WAVE = cat(tiles8<4, 4, 6, 7>(), tiles8<8, 4, 6, 7>());
