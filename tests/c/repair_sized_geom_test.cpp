// Stand-alone check of the geometry ec_repair_segments_sized lays its passes out
// with (uplink_amd/csrc/sized_geom.hpp, share_max_tiles of rs_rows.hpp; no HIP):
// repair has a fourth wave-count class, 8 waves, next to Rebuild's 2, 3 and 4.
// Every tile of every segment must lie in exactly one launch, under the map
// entry the segment's prep workgroup fills, with tile0 / map_off consistent --
// for the real launch limits, for a small fake limit that cuts a class into
// several launches, and with the classes in mixed order.  Compiled with
// -fsanitize=address,undefined and run by tests/test_repair_sized_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rs_rows.hpp"
#include "sized_geom.hpp"

using namespace uplink_ec;
using namespace uplink_ec::sized;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            failures++;                                              \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)

// repair_waves (rs_repair.hip), restated: the class of a segment with `rows` computed rows
static int waves_of(int rows) { return rows <= 14 ? 2 : rows <= 24 ? 3 : rows <= 32 ? 4 : 8; }

// What the prep kernel and the launches do with a layout, played on the host: the map filled per
// segment at map_off + tile0, then every launch's tiles looked up as the kernel looks them up.
// Each (segment, tile) must be visited exactly once, by a launch of the segment's own class.
template <class F>
static void play(const std::vector<int> &nw, const std::vector<int64_t> &tiles, F &&max_tiles) {
    const size_t n = nw.size();
    const Layout L = layout(nw.data(), tiles.data(), n, max_tiles);
    CHECK(L.idx.size() == n && L.tile0.size() == n && L.map_off.size() == n);
    int64_t total = 0;
    for (int64_t t : tiles) total += t;
    CHECK(L.map_entries == total);
    std::vector<int64_t> map((size_t)total, -1);
    std::vector<char> placed(n, 0);
    for (size_t q = 0; q < n; q++) {
        const int g = L.idx[q];
        CHECK(g >= 0 && (size_t)g < n && !placed[g]);
        placed[g] = 1;
        CHECK(L.tile0[q] >= 0 && L.map_off[q] >= 0 && L.map_off[q] + L.tile0[q] + tiles[g] <= total);
        for (int64_t i = 0; i < tiles[g]; i++) {
            int64_t &e = map[(size_t)(L.map_off[q] + L.tile0[q] + i)];
            CHECK(e == -1);  // no two segments share a map entry
            e = (int64_t)q;
        }
    }
    for (int64_t e : map) CHECK(e >= 0);
    std::vector<std::vector<int>> visits(n);
    for (size_t q = 0; q < n; q++) visits[q].assign((size_t)tiles[L.idx[q]], 0);
    for (const Launch &ln : L.launches) {
        CHECK(ln.tiles > 0 && ln.tiles <= max_tiles(ln.nw) && ln.tile_base >= 0);
        CHECK(ln.map_off >= 0 && ln.map_off + ln.tile_base + ln.tiles <= total);
        for (int64_t b = 0; b < ln.tiles; b++) {
            const int64_t ctile = ln.tile_base + b;      // a.tile_base + blockIdx.x
            const int64_t q = map[(size_t)(ln.map_off + ctile)];  // a.map[ctile]
            const int64_t tile = ctile - L.tile0[(size_t)q];       // the geometry's tile within the segment
            CHECK(nw[L.idx[(size_t)q]] == ln.nw);
            CHECK(L.map_off[(size_t)q] == ln.map_off);
            CHECK(tile >= 0 && tile < tiles[L.idx[(size_t)q]]);
            if (tile >= 0 && tile < tiles[L.idx[(size_t)q]]) visits[(size_t)q][(size_t)tile]++;
        }
    }
    for (size_t q = 0; q < n; q++)
        for (int v : visits[q]) CHECK(v == 1);
}

int main() {
    CHECK(waves_of(14) == 2 && waves_of(15) == 3 && waves_of(24) == 3 && waves_of(25) == 4 && waves_of(32) == 4 &&
          waves_of(33) == 8 && waves_of(256) == 8);
    // the launch limit: one workgroup per tile, the grid's work-items below 2^32
    for (int w : {2, 3, 4, 8}) {
        CHECK(share_max_tiles(w) * w * 64 <= 0xFFFFFFFFll);
        CHECK((share_max_tiles(w) + 1) * w * 64 > 0xFFFFFFFFll);
    }
    CHECK(share_max_tiles(8) == 8388607);
    // the tile-edge batch of tests/test_repair_sized.py: RS(29,80) ess 256, rows = targets
    {
        const std::vector<uint64_t> stripes{1, 4, 5, 7, 8, 9, 16, 17, 41, 130};
        const std::vector<int> rows{1, 51, 14, 15, 24, 25, 32, 33, 45, 8};
        std::vector<int> nw;
        std::vector<int64_t> tiles;
        for (size_t i = 0; i < stripes.size(); i++) {
            nw.push_back(waves_of(rows[i]));
            tiles.push_back(tiles_of(chunks_of(stripes[i], 256)));
        }
        CHECK((nw == std::vector<int>{2, 8, 2, 3, 3, 4, 4, 8, 8, 2}));
        play(nw, tiles, share_max_tiles);
        const Layout L = layout(nw.data(), tiles.data(), nw.size(), share_max_tiles);
        // classes in ascending order, stable within a class: 2: {0, 2, 9}, 3: {3, 4}, 4: {5, 6}, 8: {1, 7, 8}
        CHECK((L.idx == std::vector<int>{0, 2, 9, 3, 4, 5, 6, 1, 7, 8}));
        CHECK((L.tile0 == std::vector<int64_t>{0, 1, 2, 0, 1, 0, 2, 0, 1, 4}));
        CHECK((L.map_off == std::vector<int64_t>{0, 0, 0, 19, 19, 21, 21, 25, 25, 25}));
        CHECK(L.launches.size() == 4 && L.launches[3].nw == 8 && L.launches[3].tiles == 10 &&
              L.launches[3].map_off == 25 && L.launches[3].tile_base == 0);
        // the reverse order of the call: the same classes, each in reverse
        std::vector<int> rnw(nw.rbegin(), nw.rend());
        std::vector<int64_t> rtiles(tiles.rbegin(), tiles.rend());
        play(rnw, rtiles, share_max_tiles);
    }
    // a class larger than one launch: a fake limit of 5 tiles (3 on 8 waves), classes in mixed order;
    // segments straddle launches
    {
        const std::vector<int> nw{8, 2, 8, 4, 2, 8, 3, 8, 2};
        const std::vector<int64_t> tiles{7, 3, 1, 6, 9, 4, 2, 5, 1};
        auto lim = [](int w) { return (int64_t)(w == 8 ? 3 : 5); };
        play(nw, tiles, lim);
        const Layout L = layout(nw.data(), tiles.data(), nw.size(), lim);
        // 2 waves: 13 tiles in 5 + 5 + 3; 3 waves: 2; 4 waves: 6 in 5 + 1; 8 waves: 17 in 3 x 5 + 2
        CHECK(L.launches.size() == 3 + 1 + 2 + 6);
        CHECK(L.launches[6].nw == 8 && L.launches[6].map_off == 21 && L.launches[11].tile_base == 15 &&
              L.launches[11].tiles == 2);
        // a limit of one tile: a launch per tile
        play(nw, tiles, [](int) { return (int64_t)1; });
    }
    // only the 8-wave class; segments of no tiles in between (skipped segments never reach a pass,
    // but the layout must not mind)
    play({8, 8, 8}, {4, 0, 2}, [](int) { return (int64_t)4; });
    play({8}, {1}, share_max_tiles);
    // the pass split of a repair queue: 1030 one- and two-tile segments, then one past kPassTiles
    {
        std::vector<int64_t> t;
        for (int i = 0; i < 1030; i++) t.push_back(1 + i % 2);
        std::vector<Pass> p = split_passes(t.data(), t.size(), kPassSegs, kPassTiles);
        CHECK(p.size() == 2 && p[0].i0 == 0 && p[0].i1 == kPassSegs && p[1].i0 == kPassSegs && p[1].i1 == 1030);
        t.push_back(kPassTiles + 1);
        t.push_back(1);
        p = split_passes(t.data(), t.size(), kPassSegs, kPassTiles);
        CHECK(p.size() == 4 && p[2].i0 == 1030 && p[2].i1 == 1031 && p[3].i1 == 1032);
        // each pass laid out with the classes alternating
        for (const Pass &x : p) {
            if (x.i1 - x.i0 < 2) continue;
            std::vector<int> nw;
            std::vector<int64_t> tt;
            for (size_t i = x.i0; i < x.i1; i++) {
                nw.push_back(i % 3 == 0 ? 8 : i % 3 == 1 ? 2 : 4);
                tt.push_back(t[i]);
            }
            play(nw, tt, [](int w) { return (int64_t)(w == 8 ? 100 : 1000); });
        }
    }
    // the chunk limit of a segment: ess 256 is 16 chunks per stripe
    CHECK(chunks_of((uint64_t)1 << 28, 256) == -1 && chunks_of(((uint64_t)1 << 28) - 1, 256) == 0xFFFFFFF0ll);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
