// fill_bits.cpp -- CPU test of the two host/device headers of the native 3-phase assembly (stand-alone, built with
// -fsanitize=address,undefined by tests/test_fill_bits.py).
//   Part one: csrc/fill_step.hpp run on the host as a whole flood fill -- the single-workgroup form (the image's bitmaps in
//   one array, periodic inside) and the tiled form (row tiles of 1..8 rows with a one-row halo read from the global bitmap,
//   launch after launch until a launch changes nothing) -- against deff::flood_fill, Grid and PathFlag.
//   Part two: csrc/row_index3.hpp -- the row numbering is dense and injective, ends at 451, ignores neighbours the position
//   class has no link to, and every table row is fvm_row of its tuple, byte for byte.
// usage: fill_bits <random masks> <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "fill_step.hpp"
#include "flood_fill.hpp"
#include "row_index3.hpp"

using namespace deff;

static int g_fail = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                    \
            std::printf("\n");                           \
            if (++g_fail > 20) std::exit(1);             \
        }                                                \
    } while (0)

struct Mask {
    int nx, ny;
    std::vector<uint8_t> solid;                          // [ny][nx]
    std::string name;
};

struct Bitmaps {
    int nw;
    std::vector<uint64_t> open, reach;
    bool quirk;
};

static Bitmaps seed_bitmaps(const Mask &k)
{
    Bitmaps b;
    b.nw = fill_words(k.nx);
    b.open.assign((size_t)k.ny * b.nw, 0);
    b.reach.assign((size_t)k.ny * b.nw, 0);
    b.quirk = k.solid[0] != 0;
    for (int i = 0; i < k.ny; ++i)
        for (int j = 0; j < k.nx; ++j)
            if (!k.solid[(size_t)i * k.nx + j]) b.open[(size_t)i * b.nw + (j >> 6)] |= 1ull << (j & 63);
    for (int i = 0; i < k.ny; ++i)
        for (int w = 0; w < b.nw; ++w) {
            CHECK((b.open[(size_t)i * b.nw + w] & ~fill_mesh_mask(w, k.nx)) == 0, "open bit outside the mesh");
            b.reach[(size_t)i * b.nw + w] = b.open[(size_t)i * b.nw + w] & fill_seed_mask(w, k.nx, b.quirk);
        }
    return b;
}

// the rounds of one workgroup (kernels_fill.hpp: fill_rounds) over rows x nw words, words visited in index order
static long long rounds_of(const uint64_t *m, uint64_t *r, const uint64_t *above0, const uint64_t *belowL, int rows, int nw,
                           long long cap, bool *grew)
{
    long long round = 0;
    bool more = true;
    *grew = false;
    for (; more && round < cap; ++round) {
        more = false;
        for (int k = 0; k < rows * nw; ++k) {
            const uint64_t mm = m[k], own = r[k];
            if (own == mm) continue;
            const int i = k / nw, w = k - i * nw;
            const uint64_t ab = i == 0 ? above0[w] : r[k - nw];
            const uint64_t be = i == rows - 1 ? belowL[w] : r[k + nw];
            const uint64_t le = w ? r[k - 1] : 0ull, ri = w < nw - 1 ? r[k + 1] : 0ull;
            const uint64_t nv = fill_word(mm, own, ab, be, le, ri);
            CHECK((nv & ~mm) == 0 && (own & ~nv) == 0, "a round cleared a bit or left the open cells");
            if (nv != own) { r[k] = nv; more = true; }
        }
        *grew = *grew || more;
    }
    CHECK(!more, "round cap %lld reached while still changing", cap);
    return round;
}

static void compare(const Mask &k, const Bitmaps &b, const std::vector<unsigned int> &want, int want_path, const char *form, int tr)
{
    int path = b.quirk ? 1 : 0;
    for (int i = 0; i < k.ny; ++i) {
        for (int j = 0; j < k.nx; ++j) {
            const bool reached = (b.reach[(size_t)i * b.nw + (j >> 6)] >> (j & 63)) & 1ull;
            const unsigned int g = k.solid[(size_t)i * k.nx + j] ? 1u : (reached ? 0u : 2u);
            if (g != want[(size_t)i * k.nx + j]) {
                CHECK(false, "%s (%d x %d, %s, tile rows %d): Grid[%d][%d] = %u, flood_fill has %u", k.name.c_str(), k.nx, k.ny, form, tr, i,
                      j, g, want[(size_t)i * k.nx + j]);
                return;
            }
        }
        path |= (int)((b.reach[(size_t)i * b.nw + ((k.nx - 1) >> 6)] >> ((k.nx - 1) & 63)) & 1ull);
    }
    CHECK(path == want_path, "%s (%d x %d, %s, tile rows %d): PathFlag %d, flood_fill has %d", k.name.c_str(), k.nx, k.ny, form, tr, path,
          want_path);
}

static long long g_max_rounds = 0, g_max_launches = 0, g_over_budget = 0, g_fills = 0;

static void check_mask(const Mask &k)
{
    std::vector<unsigned int> want((size_t)k.nx * k.ny);
    for (size_t p = 0; p < want.size(); ++p) want[p] = k.solid[p] ? 1u : 0u;
    const int want_path = flood_fill(want.data(), k.nx, k.ny);
    {   // one workgroup: the whole image, the first row's upper neighbour is the last row
        Bitmaps b = seed_bitmaps(k);
        bool grew;
        const long long cap = fill_round_cap(k.ny, k.nx);
        const long long rounds = rounds_of(b.open.data(), b.reach.data(), b.reach.data() + (size_t)(k.ny - 1) * b.nw, b.reach.data(),
                                           k.ny, b.nw, cap, &grew);
        CHECK(rounds < cap, "rounds %lld not under the cap %lld", rounds, cap);
        g_max_rounds = std::max(g_max_rounds, rounds);
        compare(k, b, want, want_path, "one workgroup", 0);
        ++g_fills;
    }
    for (int tr = 1; tr <= 8; ++tr) {   // row tiles: local fixed points, halo rows from the global bitmap, launch after launch
        Bitmaps b = seed_bitmaps(k);
        const int nw = b.nw, ntiles = (k.ny + tr - 1) / tr;
        const long long cap = fill_round_cap(tr, k.nx);
        long long launches = 0;
        const long long sound = (long long)k.nx * k.ny + 2;          // every launch but the last sets a bit
        for (bool changed = true; changed && launches < sound; ++launches) {
            changed = false;
            for (int t = 0; t < ntiles; ++t) {
                const int r0 = t * tr, rows = std::min(tr, k.ny - r0);
                std::vector<uint64_t> m(b.open.begin() + (size_t)r0 * nw, b.open.begin() + (size_t)(r0 + rows) * nw);
                std::vector<uint64_t> r((size_t)(rows + 2) * nw);
                const int ia = r0 == 0 ? k.ny - 1 : r0 - 1, ib = r0 + rows == k.ny ? 0 : r0 + rows;
                std::memcpy(&r[0], &b.reach[(size_t)ia * nw], (size_t)nw * 8);
                std::memcpy(&r[nw], &b.reach[(size_t)r0 * nw], (size_t)rows * nw * 8);
                std::memcpy(&r[(size_t)(rows + 1) * nw], &b.reach[(size_t)ib * nw], (size_t)nw * 8);
                bool grew;
                const long long rounds = rounds_of(m.data(), &r[nw], &r[0], &r[(size_t)(rows + 1) * nw], rows, nw, cap, &grew);
                CHECK(rounds < cap, "tile rounds %lld not under the cap %lld", rounds, cap);
                g_max_rounds = std::max(g_max_rounds, rounds);
                if (grew) {
                    std::memcpy(&b.reach[(size_t)r0 * nw], &r[nw], (size_t)rows * nw * 8);
                    changed = true;
                }
            }
        }
        CHECK(launches < sound, "launches %lld not under %lld", launches, sound);
        g_max_launches = std::max(g_max_launches, launches);
        if (launches > fill_launch_cap(k.ny, k.nx)) ++g_over_budget;   // the library hands such an image to the host fill
        compare(k, b, want, want_path, "tiles", tr);
        ++g_fills;
    }
}

static Mask blank(int nx, int ny, uint8_t v, const char *name) { return Mask{nx, ny, std::vector<uint8_t>((size_t)nx * ny, v), name}; }

static void designed(int nx, int ny)
{
    {   // serpentine: one seed (the top-left cell), open rows joined alternately at the right and the left end: the path is
        // about ny nx / 2 long
        Mask k = blank(nx, ny, 1, "serpentine by rows");
        k.solid[0] = 0;
        for (int i = 0; i < ny; i += 2)
            for (int j = 1; j < nx; ++j) k.solid[(size_t)i * nx + j] = 0;
        for (int i = 1; i < ny; i += 2) k.solid[(size_t)i * nx + (((i / 2) & 1) ? 1 : nx - 1)] = 0;
        check_mask(k);
    }
    {   // serpentine by columns: every vertical step costs the word fill a round
        Mask k = blank(nx, ny, 1, "serpentine by columns");
        for (int j = 0; j < nx; j += 2)
            for (int i = 1; i < ny - 1; ++i) k.solid[(size_t)i * nx + j] = 0;
        for (int j = 1; j < nx; j += 2) k.solid[(size_t)(((j / 2) & 1) ? 1 : ny - 2) * nx + j] = 0;
        if (ny > 3) check_mask(k);
    }
    if (nx >= 3 && ny >= 4) {   // a pore reachable only through the wrap between row 0 and row ny - 1
        Mask k = blank(nx, ny, 1, "wrap only");
        for (int j = 0; j < nx; ++j) k.solid[(size_t)(ny - 1) * nx + j] = 0;          // last row open, seeded at column 0
        k.solid[nx - 1] = 0;                                                          // row 0, last column: joins through the wrap
        k.solid[(size_t)1 * nx + nx - 1] = 0;                                         // and goes on down
        k.solid[0] = 0;
        k.solid[1] = 1;
        check_mask(k);
    }
    {   // solid left column: nothing is seeded, every pore is 2, PathFlag 0 -- except through the quirk, so keep (0, 0) open
        Mask k = blank(nx, ny, 0, "solid left column");
        for (int i = 1; i < ny; ++i) k.solid[(size_t)i * nx] = 1;
        if (nx > 1) k.solid[1] = 1;
        if (ny > 1 && nx > 1) k.solid[(size_t)(ny - 1) * nx] = 1;
        check_mask(k);
        for (int i = 0; i < ny; ++i) k.solid[(size_t)i * nx] = 1;                     // all of it: the quirk seeds the right
        k.name = "solid left column, quirk";
        check_mask(k);
    }
    check_mask(blank(nx, ny, 0, "all open"));
    check_mask(blank(nx, ny, 1, "all solid"));
    {   // the quirk with solid cells in the last column: they spread to their west neighbours and stay solid
        Mask k = blank(nx, ny, 1, "quirk, solid last column");
        for (int i = 0; i < ny; i += 2)
            for (int j = 1; j < nx - 1; ++j) k.solid[(size_t)i * nx + j] = 0;
        for (int i = 1; i < ny; i += 3) k.solid[(size_t)i * nx + nx - 1] = 0;
        check_mask(k);
    }
}

static void part_one(int count, unsigned seed)
{
    std::mt19937_64 rng(seed);
    const int widths[] = {2, 3, 63, 64, 65, 127, 128, 130, 258};
    for (int c = 0; c < count; ++c) {
        Mask k;
        k.nx = widths[rng() % 9];
        k.ny = 2 + (int)(rng() % 39);
        k.name = "random";
        const double frac = 0.2 + 0.7 * (double)(rng() % 1000) / 999.0;
        k.solid.resize((size_t)k.nx * k.ny);
        for (auto &v : k.solid) v = (double)(rng() % 100000) / 100000.0 < frac;
        k.solid[0] = (c % 3) == 0;                       // a third with the top-left cell solid
        check_mask(k);
    }
    for (int nx : widths)
        for (int ny : {2, 3, 7, 16, 40}) designed(nx, ny);
    std::printf("part one: %lld fills equal to flood_fill; most rounds of a workgroup %lld, most launches of the tiled form %lld, "
                "%lld tiled fills over the launch budget\n", g_fills, g_max_rounds, g_max_launches, g_over_budget);
}

static void part_two()
{
    std::set<int> seen;
    int lo = 1 << 30, hi = -1, tuples = 0;
    std::vector<double> rows((size_t)NATIVE3_ROWS * 6);
    const double Ds = 1e-3, Df = 1.0, Dg = 1e4, dx = 1.0 / 37, dy = 1.0 / 29, CL = 2.0, CR = -1.0;
    build_rows3(rows.data(), Ds, Df, Dg, dx, dy, CL, CR);
    const double Dn[3] = {Df, Ds, Dg}, Do[2] = {Df, Dg};
    for (int ycls = 0; ycls < 3; ++ycls)
        for (int xcls = 0; xcls < 3; ++xcls) {
            std::set<int> cls_rows;
            std::set<std::vector<int>> admissible;       // tuples reduced to the neighbours the class has links to
            for (int own = 0; own < 2; ++own)
                for (int cw = 0; cw < 3; ++cw)
                    for (int ce = 0; ce < 3; ++ce)
                        for (int cs = 0; cs < 3; ++cs)
                            for (int cn = 0; cn < 3; ++cn) {
                                const int row = native3_row(ycls, xcls, own, cw, ce, cs, cn);
                                ++tuples;
                                lo = std::min(lo, row); hi = std::max(hi, row);
                                const std::vector<int> key = {own, xcls != POS_FIRST ? cw : -1, xcls != POS_LAST ? ce : -1,
                                                              ycls != POS_LAST ? cs : -1, ycls != POS_FIRST ? cn : -1};
                                const bool fresh_key = admissible.insert(key).second, fresh_row = cls_rows.insert(row).second;
                                CHECK(fresh_key == fresh_row, "class (%d, %d): row %d and its tuple disagree on being new", ycls, xcls, row);
                                // the same row whatever a neighbour without a link is
                                CHECK(row == native3_row(ycls, xcls, own, xcls == POS_FIRST ? 0 : cw, xcls == POS_LAST ? 2 : ce,
                                                         ycls == POS_LAST ? 1 : cs, ycls == POS_FIRST ? 2 : cn),
                                      "class (%d, %d): a neighbour without a link enters the row", ycls, xcls);
                                const FvmRow r = fvm_row(Do[own], Dn[cw], Dn[ce], Dn[cs], Dn[cn], xcls, ycls, dx, dy, CL, CR);
                                const double want[6] = {r.a0, r.aW, r.aE, r.aS, r.aN, r.b};
                                CHECK(!std::memcmp(want, &rows[(size_t)row * 6], sizeof want), "row %d is not fvm_row of its tuple", row);
                            }
            CHECK((int)cls_rows.size() == native3_class_rows(ycls, xcls), "class (%d, %d) has %zu rows", ycls, xcls, cls_rows.size());
            CHECK(*cls_rows.begin() == native3_class_base(ycls, xcls) &&
                      *cls_rows.rbegin() == native3_class_base(ycls, xcls) + native3_class_rows(ycls, xcls) - 1,
                  "class (%d, %d) is not dense", ycls, xcls);
            for (int row : cls_rows) CHECK(seen.insert(row).second, "row %d belongs to two classes", row);
        }
    CHECK(lo == NATIVE3_FIRST && hi == 451 && hi == NATIVE3_ROWS - 1 && (int)seen.size() == 450, "rows %d .. %d, %zu of them", lo, hi,
          seen.size());
    const double zero[6] = {0, 0, 0, 0, 0, 0}, ident[6] = {1, 0, 0, 0, 0, 0};
    CHECK(!std::memcmp(zero, &rows[0], sizeof zero) && !std::memcmp(ident, &rows[6], sizeof ident), "rows 0 and 1");
    std::printf("part two: %d tuples name %zu rows, %d .. %d, dense and injective, each fvm_row of its tuple\n", tuples, seen.size(), lo, hi);
}

int main(int argc, char **argv)
{
    const int count = argc > 1 ? std::atoi(argv[1]) : 200;
    const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    part_one(count, seed);
    part_two();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
