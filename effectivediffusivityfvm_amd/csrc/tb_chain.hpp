// tb_chain.hpp -- who waits for whom when the streaming kernel chains passes inside one launch (k_sweep_matfree_tb_chain,
// kernels_tb.hpp).  Host only, no HIP: a pure function of the dealt table and the geometry, so that it can be checked on a CPU
// against a cell-by-cell brute force (tests/cpp/tb_chain_lists.cpp).
//
// A tile is one entry of the dealt table (deal_ranked_tiles, api_sweep.hip): strip tx of image img, rows [ry0, ry0 + rows).
// In a pass, tb_strip
//   loads   window(tile) = columns [tx * WOUT - shift, + 128) inside [0, nx)  x  rows [max(ry0 - T, row_lo), min(ry1 + T, row_hi)),
//   stores  own(tile)    = columns [out_lo, out_hi) of the window            x  rows [ry0, ry1),
// with row_lo / row_hi the image's mesh rows, ry1 = min(ry0 + rows, own_hi), out_lo / out_hi as in tb_strip.
// Tile n is a neighbour of tile t when  own(n) meets window(t)  -- n produces what t reads next pass --  or  window(n) meets
// own(t)  -- n still reads the buffer t overwrites next pass.  The relation is symmetric by construction.  Before pass p > 0 a
// tile waits until every neighbour has published pass p - 1: both hazards are covered by that one wait.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace deff {

constexpr int TB_CHAIN_MAXN = 16;                        // neighbours per tile the device table holds
constexpr int TB_CHAIN_COLS = 128;                       // = TB_COLS (kernels_tb.hpp; static_assert there)

struct TbChainTile { int x, y, z, w; };                  // an entry of the dealt table, laid out as its int4: tx | img << 16, ry0, rows, stamp
struct TbChainRect { int c0, c1, r0, r1; };              // columns [c0, c1) x rows [r0, r1)
struct TbChainGeom {
    int nx, T, shift, ntx;
    int pitch;                                           // rows between two images of a stack
    int dom_lo, ny;                                      // image k: mesh rows [dom_lo + k * pitch, + ny)
    int own_lo, own_h;                                   //          owned rows [own_lo + k * pitch, + own_h)
};

inline bool tb_chain_meet(const TbChainRect &a, const TbChainRect &b)
{
    return std::max(a.c0, b.c0) < std::min(a.c1, b.c1) && std::max(a.r0, b.r0) < std::min(a.r1, b.r1);
}

// what tb_strip loads and stores for this table entry (empty rectangles for an entry without rows)
inline void tb_chain_rects(const TbChainGeom &g, const TbChainTile &t, TbChainRect *window, TbChainRect *own)
{
    const int hw = (g.T + 1) & ~1, wout = TB_CHAIN_COLS - 2 * hw;
    const int tx = t.x & 0xFFFF, img = t.x >> 16;
    const int row_lo = g.dom_lo + img * g.pitch, row_hi = row_lo + g.ny;
    const int own_hi = g.own_lo + img * g.pitch + g.own_h;
    const int ry0 = t.y, ry1 = std::min(ry0 + t.z, own_hi);
    const int first = tx * wout - g.shift;
    window->c0 = std::max(first, 0);
    window->c1 = std::min(first + TB_CHAIN_COLS, g.nx);
    window->r0 = std::max(ry0 - g.T, row_lo);
    window->r1 = std::min(ry1 + g.T, row_hi);
    own->c0 = std::max(tx == 0 ? 0 : first + hw, window->c0);
    own->c1 = std::min(tx == g.ntx - 1 ? g.nx : first + TB_CHAIN_COLS - hw, window->c1);
    own->r0 = ry0;
    own->r1 = ry1;
    if (t.z <= 0) *window = *own = TbChainRect{0, 0, 0, 0};
}

// lists[TB_CHAIN_MAXN * k ...]: the table indices of entry k's neighbours, ascending, padded with -1.  Entries without rows
// have no list and are in nobody's.  Returns false -- the table cannot be chained -- when some tile has more than
// TB_CHAIN_MAXN neighbours; `lists` is then unspecified.
inline bool tb_chain_lists(const TbChainGeom &g, const TbChainTile *tab, size_t entries, std::vector<int> *lists)
{
    lists->assign(entries * TB_CHAIN_MAXN, -1);
    std::vector<TbChainRect> win(entries), own(entries);
    std::vector<int> order, lo(entries), hi(entries);                         // the entries with rows, by the first row they touch
    for (size_t k = 0; k < entries; ++k) {
        tb_chain_rects(g, tab[k], &win[k], &own[k]);
        lo[k] = std::min(win[k].r0, own[k].r0);
        hi[k] = std::max(win[k].r1, own[k].r1);
        if (tab[k].z > 0) order.push_back((int)k);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return lo[a] != lo[b] ? lo[a] < lo[b] : a < b; });
    std::vector<int> count(entries, 0);
    bool fits = true;
    auto add = [&](int a, int b) {
        if (count[a] < TB_CHAIN_MAXN) (*lists)[(size_t)a * TB_CHAIN_MAXN + count[a]] = b;
        else fits = false;
        ++count[a];
    };
    // every pair whose row ranges overlap is tested; images of a stack never do
    for (size_t i = 0; i < order.size(); ++i) {
        const int a = order[i];
        for (size_t j = i + 1; j < order.size() && lo[order[j]] < hi[a]; ++j) {
            const int b = order[j];
            if (tb_chain_meet(own[b], win[a]) || tb_chain_meet(win[b], own[a])) { add(a, b); add(b, a); }
        }
    }
    if (!fits) return false;
    for (size_t k = 0; k < entries; ++k) std::sort(lists->begin() + k * TB_CHAIN_MAXN, lists->begin() + k * TB_CHAIN_MAXN + count[k]);
    return true;
}

}  // namespace deff
