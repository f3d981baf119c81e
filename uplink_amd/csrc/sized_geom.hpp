// Geometry of a share-set call whose segments differ in size
// (include/uplink_ec.h ec_rebuild_segments_sized, rs_sized.hpp): tiles per
// segment, the 32-bit chunk limit, the order of a pass's segments by wave-count
// class with each segment's first tile, the launches a class is cut into, and
// the passes a call is cut into.  Plain C++, no HIP: tests/test_sized_host.py
// compiles it on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace uplink_ec {
namespace sized {

constexpr int64_t kTileChunks = 128;           // 16-byte chunks per tile (rs_tile.hpp kTileChunks)
constexpr uint64_t kMaxChunks = 0xFFFFFFFFu;   // the tile body divides chunk indices as uint32_t
// a pass's staging is bounded by its segments and by its tile map (4 bytes per tile);
// a segment larger than kPassTiles is a pass of its own
constexpr size_t kPassSegs = 1024;
constexpr int64_t kPassTiles = (int64_t)1 << 20;

// 16-byte chunks of one share of a segment of nstripes stripes, -1 when the
// count does not fit 32 bits (or nstripes * ess does not fit 64)
inline int64_t chunks_of(uint64_t nstripes, int ess) {
    if (ess <= 0) return -1;
    if (nstripes > UINT64_MAX / (uint64_t)ess) return -1;
    const uint64_t c = nstripes * (uint64_t)ess / 16;
    return c > kMaxChunks ? -1 : (int64_t)c;
}

inline int64_t tiles_of(int64_t chunks) { return (chunks + kTileChunks - 1) / kTileChunks; }

// Segments [i0, i1) of a call's list form one pass.
struct Pass {
    size_t i0, i1;
};

// Consecutive segments until a pass holds max_segs segments or adding the next
// would take it past max_tiles tiles; every pass holds at least one segment.
inline std::vector<Pass> split_passes(const int64_t *tiles, size_t n, size_t max_segs, int64_t max_tiles) {
    std::vector<Pass> out;
    size_t i0 = 0;
    int64_t sum = 0;
    for (size_t i = 0; i < n; i++) {
        if (i > i0 && (i - i0 >= max_segs || sum + tiles[i] > max_tiles)) {
            out.push_back({i0, i});
            i0 = i;
            sum = 0;
        }
        sum += tiles[i];
    }
    if (n > i0) out.push_back({i0, n});
    return out;
}

// One launch of the tile kernel: tiles [tile_base, tile_base + tiles) of the
// class on nw waves, whose map starts at entry map_off of the pass's map.
struct Launch {
    int nw;
    int64_t map_off, tile_base, tiles;
};

// A pass laid out: its segments in class order, each with its first tile in its
// class's tile numbering; one map per class, the classes' maps one after the
// other; a class of more tiles than one launch takes cut into parts.
struct Layout {
    std::vector<int> idx;          // position q holds segment idx[q] of the pass (stable by class)
    std::vector<int64_t> tile0;    // [q] first tile of that segment within its class
    std::vector<int64_t> map_off;  // [q] first entry of its class's map
    std::vector<Launch> launches;
    int64_t map_entries = 0;
};

// nw[i], tiles[i]: segment i's wave-count class and tile count; max_tiles(nw):
// most tiles one launch on nw waves takes.
template <class F>
inline Layout layout(const int *nw, const int64_t *tiles, size_t n, F &&max_tiles) {
    Layout L;
    L.idx.resize(n);
    for (size_t i = 0; i < n; i++) L.idx[i] = (int)i;
    std::stable_sort(L.idx.begin(), L.idx.end(), [&](int x, int y) { return nw[x] < nw[y]; });
    L.tile0.assign(n, 0);
    L.map_off.assign(n, 0);
    for (size_t q0 = 0; q0 < n;) {
        const int w = nw[L.idx[q0]];
        size_t q1 = q0;
        int64_t t = 0;
        for (; q1 < n && nw[L.idx[q1]] == w; q1++) {
            L.tile0[q1] = t;
            L.map_off[q1] = L.map_entries;
            t += tiles[L.idx[q1]];
        }
        const int64_t per = max_tiles(w);
        for (int64_t b = 0; b < t; b += per) L.launches.push_back({w, L.map_entries, b, std::min(per, t - b)});
        L.map_entries += t;
        q0 = q1;
    }
    return L;
}

}  // namespace sized
}  // namespace uplink_ec
