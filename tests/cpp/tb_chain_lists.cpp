// The neighbour lists of a chained streaming launch (csrc/tb_chain.hpp) against a cell-by-cell brute force, on random tile
// tables.  CPU only; built with -fsanitize=address,undefined by tests/test_tb_chain_lists.py.
//   tb_chain_lists [tables] [seed]
// The brute force walks what tb_strip (kernels_tb.hpp) does lane by lane: which cells a tile's lanes load, which they store.
// It paints every cell with the tile that stores it, then collects, for every tile, the owners of the cells it loads; n is a
// neighbour of t when n owns a cell t loads or t owns a cell n loads.
#include "tb_chain.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using namespace deff;

struct Table {
    TbChainGeom g;
    int nimg;
    std::vector<TbChainTile> tab;
};

// lane by lane, as tb_strip: fn(row, col) for every cell loaded (LOADS) or stored
template <bool LOADS, class F> static void cells_of(const TbChainGeom &g, const TbChainTile &t, F fn)
{
    if (t.z <= 0) return;
    const int T = g.T, HW = (T + 1) & ~1, WOUT = 128 - 2 * HW;
    const int tx = t.x & 0xFFFF, img = t.x >> 16;
    const int row_lo = g.dom_lo + img * g.pitch, row_hi = row_lo + g.ny, own_hi = g.own_lo + img * g.pitch + g.own_h;
    const int ry0 = t.y, ry1 = std::min(ry0 + t.z, own_hi);
    const int r_begin = std::max(ry0 - T, row_lo), r_end = ry1 + T, win_hi = std::min(r_end, row_hi);
    const int out_lo = tx == 0 ? 0 : tx * WOUT - g.shift + HW;
    const int out_hi = tx == g.ntx - 1 ? g.nx : tx * WOUT - g.shift + 128 - HW;
    for (int lane = 0; lane < 64; ++lane) {
        const int col = tx * WOUT - g.shift + 2 * lane;
        const bool in_x = col >= 0 && col < g.nx;
        const bool st_x = in_x && col >= out_lo && col < out_hi;
        if (LOADS) {
            if (!in_x) continue;
            for (int r = r_begin; r < win_hi; ++r) { fn(r, col); fn(r, col + 1); }
        } else {
            if (!st_x) continue;
            for (int r = ry0; r < ry1; ++r) { fn(r, col); fn(r, col + 1); }
        }
    }
}

static Table draw(std::mt19937 &rng, bool crowded)
{
    auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    Table t;
    const int Ts[5] = {8, 8, 6, 4, 2};
    const int T = Ts[pick(0, 4)], hw = (T + 1) & ~1, wout = 128 - 2 * hw;
    const int strips = pick(1, 12);
    const bool place_b = pick(0, 1) != 0;                                       // no halo outside a wall (shift = 0) or the older placement
    // ragged nx (even) with exactly `strips` strips under the chosen placement (plan_strips, api_sweep.hip)
    int nx;
    if (place_b) nx = strips == 1 ? 2 * pick(1, 64) : 128 + (strips - 2) * wout + 2 * pick(1, wout / 2);
    else nx = (strips - 1) * wout + 2 * pick(1, wout / 2);
    t.nimg = pick(1, 3);
    const int ny = pick(T, crowded ? 40 * T : 12 * T);
    t.g = TbChainGeom{nx, T, place_b ? 0 : hw, strips, ny, 0, ny, 0, ny};
    for (int img = 0; img < t.nimg; ++img)
        for (int tx = 0; tx < strips; ++tx) {
            // random cuts of at least T rows; `crowded` puts one tall chunk beside many short ones
            int r = 0;
            const bool tall = crowded && tx % 2 == 0;
            while (r < ny) {
                int h = tall ? ny : pick(T, crowded ? T + 1 : 3 * T);
                if (ny - (r + h) < T) h = ny - r;
                t.tab.push_back(TbChainTile{tx | (img << 16), img * ny + r, h, 0});
                r += h;
            }
        }
    for (int k = pick(0, 5); k > 0; --k) t.tab.push_back(TbChainTile{pick(0, strips - 1), pick(0, ny - 1), 0, 0});   // waves without a tile
    std::shuffle(t.tab.begin(), t.tab.end(), rng);
    return t;
}

static int fail(const Table &t, const char *what, int a, int b)
{
    std::fprintf(stderr, "FAIL: %s (tiles %d, %d): nx %d T %d shift %d strips %d images %d ny %d, %zu entries\n", what, a, b, t.g.nx, t.g.T,
                 t.g.shift, t.g.ntx, t.nimg, t.g.ny, t.tab.size());
    return 1;
}

static int check(const Table &t, long *fitted, long *refused)
{
    const TbChainGeom &g = t.g;
    const int rows = g.pitch * t.nimg, n = (int)t.tab.size();
    std::vector<int> owner((size_t)rows * g.nx, -1);
    for (int k = 0; k < n; ++k) {
        int clash = -1;
        cells_of<false>(g, t.tab[k], [&](int r, int c) {
            int &o = owner[(size_t)r * g.nx + c];
            if (o >= 0) clash = o;
            o = k;
        });
        if (clash >= 0) return fail(t, "two tiles store one cell", k, clash);
    }
    for (int o : owner)
        if (o < 0) return fail(t, "a cell nobody stores", -1, -1);
    std::vector<std::set<int>> want(n);
    for (int k = 0; k < n; ++k)
        cells_of<true>(g, t.tab[k], [&](int r, int c) {
            const int o = owner[(size_t)r * g.nx + c];
            if (o != k) { want[k].insert(o); want[o].insert(k); }
        });
    size_t most = 0;
    for (int k = 0; k < n; ++k) most = std::max(most, want[k].size());
    std::vector<int> lists;
    const bool fits = tb_chain_lists(g, t.tab.data(), t.tab.size(), &lists);
    if (fits != (most <= (size_t)TB_CHAIN_MAXN)) return fail(t, fits ? "lists reported to fit that do not" : "lists reported not to fit that do", (int)most, 0);
    if (!fits) { ++*refused; return 0; }
    ++*fitted;
    if (lists.size() != (size_t)n * TB_CHAIN_MAXN) return fail(t, "list table of the wrong size", (int)lists.size(), n);
    for (int k = 0; k < n; ++k) {
        std::set<int> got;
        for (int i = 0; i < TB_CHAIN_MAXN; ++i) {
            const int v = lists[(size_t)k * TB_CHAIN_MAXN + i];
            if (v < -1 || v >= n) return fail(t, "index out of the table", k, v);
            if (v >= 0) {
                if (i > 0 && lists[(size_t)k * TB_CHAIN_MAXN + i - 1] < 0) return fail(t, "entry behind the padding", k, v);
                if (!got.insert(v).second) return fail(t, "neighbour listed twice", k, v);
                if (t.tab[v].z <= 0) return fail(t, "a wave without a tile is listed", k, v);
            }
        }
        if (t.tab[k].z <= 0 && !got.empty()) return fail(t, "a wave without a tile has a list", k, 0);
        if (got != want[k]) return fail(t, "list differs from the brute force", k, (int)got.size() - (int)want[k].size());
        if (got.count(k)) return fail(t, "tile lists itself", k, k);
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int tables = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 20260u);
    long fitted = 0, refused = 0;
    for (int k = 0; k < tables; ++k)
        if (check(draw(rng, k % 5 == 4), &fitted, &refused)) return 1;
    // one table made to overflow: a tall chunk beside T-row chunks of the next strip
    {
        Table t;
        const int T = 8, ny = 40 * T;
        t.nimg = 1;
        t.g = TbChainGeom{200, T, 0, 2, ny, 0, ny, 0, ny};
        t.tab.push_back(TbChainTile{0, 0, ny, 0});
        for (int r = 0; r < ny; r += T) t.tab.push_back(TbChainTile{1, r, T, 0});
        std::vector<int> lists;
        if (tb_chain_lists(t.g, t.tab.data(), t.tab.size(), &lists)) return fail(t, "a tile with 40 neighbours was reported to fit", 0, 0);
        long a = 0, b = 0;
        if (check(t, &a, &b) || b != 1) return fail(t, "overflowing table", 0, 0);
    }
    if (fitted < tables / 4 || refused < 1) { std::fprintf(stderr, "FAIL: %ld tables fitted, %ld refused: the draw is lopsided\n", fitted, refused); return 1; }
    std::printf("%d tables: %ld with lists equal to the brute force, %ld correctly refused\n", tables, fitted, refused);
    return 0;
}
