// Stand-alone check of uplink_amd/csrc/sized_geom.hpp (no HIP): tile counts and
// tile bases for the stripe lists tests/test_sized.py runs, the split of a class
// into launches at a synthetic grid limit, the split of a call into passes, and
// the 32-bit chunk limit.  Compiled with -fsanitize=address,undefined and run by
// tests/test_sized_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sized_geom.hpp"

using namespace uplink_ec::sized;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            failures++;                                              \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)

static std::vector<int64_t> tiles_for(const std::vector<uint64_t> &stripes, int ess) {
    std::vector<int64_t> t;
    for (uint64_t s : stripes) t.push_back(tiles_of(chunks_of(s, ess)));
    return t;
}

// every tile of every class belongs to exactly one segment, in order, and the launches cover each class once
static void check_layout(const Layout &L, const std::vector<int> &nw, const std::vector<int64_t> &tiles, int64_t limit) {
    const size_t n = nw.size();
    CHECK(L.idx.size() == n && L.tile0.size() == n && L.map_off.size() == n);
    std::vector<char> seen(n, 0);
    int64_t total = 0;
    for (size_t q = 0; q < n; q++) {
        CHECK(!seen[L.idx[q]]);
        seen[L.idx[q]] = 1;
        total += tiles[L.idx[q]];
        if (q > 0) {
            CHECK(nw[L.idx[q - 1]] <= nw[L.idx[q]]);
            if (nw[L.idx[q - 1]] == nw[L.idx[q]]) {
                CHECK(L.idx[q - 1] < L.idx[q]);  // stable
                CHECK(L.tile0[q] == L.tile0[q - 1] + tiles[L.idx[q - 1]]);
                CHECK(L.map_off[q] == L.map_off[q - 1]);
            } else {
                CHECK(L.tile0[q] == 0);
                CHECK(L.map_off[q] == L.map_off[q - 1] + L.tile0[q - 1] + tiles[L.idx[q - 1]]);
            }
        } else {
            CHECK(L.tile0[q] == 0 && L.map_off[q] == 0);
        }
    }
    CHECK(L.map_entries == total);
    int64_t covered = 0;
    for (size_t i = 0; i < L.launches.size(); i++) {
        const Launch &ln = L.launches[i];
        CHECK(ln.tiles > 0 && ln.tiles <= limit);
        if (i > 0 && L.launches[i - 1].nw == ln.nw) {
            CHECK(ln.map_off == L.launches[i - 1].map_off);
            CHECK(ln.tile_base == L.launches[i - 1].tile_base + L.launches[i - 1].tiles);
        } else {
            CHECK(ln.tile_base == 0 && ln.map_off == covered);
        }
        covered = ln.map_off + ln.tile_base + ln.tiles;
    }
    CHECK(covered == total);
}

int main() {
    // tiles: RS(29,80) ess 256 is 16 chunks per stripe, 8 stripes per tile
    {
        const std::vector<uint64_t> s{1, 4, 5, 7, 8, 9, 16, 17, 41, 0, 130};
        const std::vector<int64_t> want{1, 1, 1, 1, 1, 2, 2, 3, 6, 0, 17};
        CHECK(tiles_for(s, 256) == want);
        CHECK(chunks_of(4, 256) == 64 && chunks_of(5, 256) == 80);  // the vB boundary
    }
    CHECK((tiles_for({1, 2, 3}, 4096) == std::vector<int64_t>{2, 4, 6}));          // a tile is half a stripe
    CHECK((tiles_for({1, 31, 32, 33, 257}, 64) == std::vector<int64_t>{1, 1, 1, 2, 9}));  // 32 stripes
    CHECK((tiles_for({3, 1}, 16) == std::vector<int64_t>{1, 1}));
    CHECK(tiles_of(chunks_of(9060, 256)) == 1133);  // the production 64 MiB segment
    // tile bases: one class
    {
        const std::vector<int64_t> t = tiles_for({1, 4, 5, 7, 8, 9, 16, 17, 41, 130}, 256);
        const std::vector<int> nw(t.size(), 3);
        const Layout L = layout(nw.data(), t.data(), t.size(), [](int) { return (int64_t)1 << 24; });
        check_layout(L, nw, t, (int64_t)1 << 24);
        const std::vector<int64_t> want{0, 1, 2, 3, 4, 5, 7, 9, 12, 18};
        CHECK(L.tile0 == want);
        CHECK(L.launches.size() == 1 && L.launches[0].tiles == 35 && L.launches[0].nw == 3);
    }
    // three classes interleaved in the call, a map per class
    {
        const std::vector<int> nw{4, 2, 3, 2, 4, 3, 2};
        const std::vector<int64_t> t{6, 1, 2, 3, 1, 17, 2};
        const Layout L = layout(nw.data(), t.data(), nw.size(), [](int) { return (int64_t)1000; });
        check_layout(L, nw, t, 1000);
        CHECK((L.idx == std::vector<int>{1, 3, 6, 2, 5, 0, 4}));
        CHECK((L.tile0 == std::vector<int64_t>{0, 1, 4, 0, 2, 0, 6}));
        CHECK((L.map_off == std::vector<int64_t>{0, 0, 0, 6, 6, 25, 25}));
        CHECK(L.launches.size() == 3 && L.map_entries == 32);
    }
    // the part split at a synthetic grid limit of 5 tiles (3 for the 4-wave class): a
    // segment may straddle two launches
    {
        const std::vector<int> nw{2, 2, 4, 2, 4};
        const std::vector<int64_t> t{3, 6, 7, 2, 1};
        auto lim = [](int w) { return (int64_t)(w == 4 ? 3 : 5); };
        const Layout L = layout(nw.data(), t.data(), nw.size(), lim);
        check_layout(L, nw, t, 5);
        CHECK(L.launches.size() == 3 + 3);
        CHECK(L.launches[0].tiles == 5 && L.launches[1].tiles == 5 && L.launches[2].tiles == 1);
        CHECK(L.launches[1].tile_base == 5 && L.launches[2].tile_base == 10);
        CHECK(L.launches[3].nw == 4 && L.launches[3].map_off == 11 && L.launches[5].tiles == 2);
    }
    // an empty pass
    {
        const Layout L = layout((const int *)nullptr, (const int64_t *)nullptr, 0, [](int) { return (int64_t)1; });
        CHECK(L.launches.empty() && L.map_entries == 0);
    }
    // the pass split: by segments, by tiles, a segment larger than the limit on its own
    {
        const std::vector<int64_t> t{1, 1, 1, 1, 1, 1, 1};
        const std::vector<Pass> p = split_passes(t.data(), t.size(), 3, 100);
        CHECK(p.size() == 3 && p[0].i0 == 0 && p[0].i1 == 3 && p[1].i1 == 6 && p[2].i0 == 6 && p[2].i1 == 7);
        const std::vector<int64_t> u{4, 4, 4, 50, 1, 9, 1};
        const std::vector<Pass> r = split_passes(u.data(), u.size(), 100, 10);
        // {4,4} {4} {50} {1,9} {1}
        CHECK(r.size() == 5 && r[0].i1 == 2 && r[1].i1 == 3 && r[2].i1 == 4 && r[3].i1 == 6 && r[4].i1 == 7);
        size_t at = 0;
        for (const Pass &x : r) {
            CHECK(x.i0 == at && x.i1 > x.i0);
            at = x.i1;
        }
        CHECK(split_passes(t.data(), 0, 3, 100).empty());
        // thousands of small segments: passes of kPassSegs
        const std::vector<int64_t> many(5000, 1);
        CHECK(split_passes(many.data(), many.size(), kPassSegs, kPassTiles).size() == (5000 + kPassSegs - 1) / kPassSegs);
    }
    // the 32-bit chunk limit
    CHECK(chunks_of(0, 256) == 0);
    CHECK(chunks_of(0x0FFFFFFFull, 256) == 0xFFFFFFF0ll);   // 16 chunks per stripe
    CHECK(chunks_of(0x10000000ull, 256) == -1);              // 2^32 chunks
    CHECK(chunks_of(0xFFFFFFFFull, 16) == 0xFFFFFFFFll);
    CHECK(chunks_of(0x100000000ull, 16) == -1);
    CHECK(chunks_of(UINT64_MAX, 256) == -1);                 // the product does not fit 64 bits
    CHECK(chunks_of(UINT64_MAX / 256 + 1, 256) == -1);
    CHECK(chunks_of(3, 100) == 18 && chunks_of(1, 0) == -1);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
