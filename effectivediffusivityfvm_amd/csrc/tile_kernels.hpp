// tile_kernels.hpp -- the workgroup-tile kernels of a temporally blocked pass (kernels_wgtile.hpp), each instantiation listed
// once: what a list entry says about its kernel, the helpers that build the lists, and the three lists themselves.  Every
// family is instantiated in a translation unit of its own (tiles_8wave.hip, tiles_tall.hip, tiles_12wave.hip: they compile side
// by side, and nothing else has to be compiled again when a planner or a solve loop changes); api_sweep.hip plans with the
// lists and launches from them.  The planner takes its candidates from these lists and sizes a grid with the occupancy of the
// kernel it would launch; a plan names its list entry and the launchers take the kernel from there.  So a shape the planner
// can pick always has a kernel.
#pragma once
#include "kernels_wgtile.hpp"
#include <array>

using namespace deff;

// make(f) for a compile-time flag f = false, true; make(f, g) for the four pairs, at index 2 f + g.  The flags come as TbTag
// (kernels_tb.hpp): decltype(f)::value.
template <class Make> static constexpr auto by_flag(Make make) { return std::array{make(TbTag<false>{}), make(TbTag<true>{})}; }
template <class Make> static constexpr auto by_flags(Make make)
{
    return std::array{make(TbTag<false>{}, TbTag<false>{}), make(TbTag<false>{}, TbTag<true>{}), make(TbTag<true>{}, TbTag<false>{}),
                      make(TbTag<true>{}, TbTag<true>{})};
}
template <class E, size_t... N> static constexpr auto cat(const std::array<E, N> &...parts)
{
    std::array<E, (N + ...)> all{};
    size_t k = 0;
    auto put = [&](const auto &part) { for (const E &e : part) all[k++] = e; };
    (put(parts), ...);
    return all;
}

// Every resident kernel takes the argument list launch_resident (api_sweep.hip) passes.
using ResidentKernel = decltype(&k_sweep_wgsym<8, 4, false>);
using PassKernel = decltype(&k_sweep_wgtile<8, 4, false, false>);
struct TileKernel {
    int NW = 0, T = 0;                // waves per tile, sweeps per pass
    int rows[4] = {0, 0, 0, 0};       // rows of a wave by its age (wave >> 2: a SIMD serves its waves oldest first); NW / 4 ages
    int R = 0;                        // deff_get_plan("tb_R"): the oldest wave's rows, a tall tile's rows / 16
    bool fma = false, guard = false;
    bool sym = false;                 // for link-symmetric systems only (the 7-lookup short-cut)
    ResidentKernel kernel = nullptr;  // resident passes
    PassKernel pass = nullptr;        // one launch per pass: 8-wave tiles only
    constexpr int threads() const { return NW * 64; }
    constexpr int tile_rows() const { return 4 * (rows[0] + rows[1] + rows[2] + rows[3]); }
    constexpr bool aged() const { return rows[0] != rows[NW / 4 - 1]; }
};

// The lists, one family (one NW) each.  Within a form and T the planners take the first entry that fits, so each list runs
// from the fewest rows up, and whoever looks through all of them (find_tile, api_sweep.hip) goes in this order.
extern const std::array<TileKernel, 24> TILES_8WAVE;     // T = 4, then T = 8
extern const std::array<TileKernel, 98> TILES_TALL;      // equal rows, then rows by age
extern const std::array<TileKernel, 18> TILES_12WAVE;    // T = 8, 6, 4
