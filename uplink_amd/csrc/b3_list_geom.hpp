// Geometry of a BLAKE3 call over a list of pieces that each have their own
// length (include/uplink_ec.h ec_blake3_pieces_list, ec_hash_segments_sized;
// kernels in blake3.hip): chunks and 256-chunk groups per piece, each piece's
// first workgroup and first node slot in a pass, the workgroup -> piece map, the
// fast / byte / oversize classification per piece, and the passes a long list is
// cut into.  Plain C++, no HIP: tests/test_hash_sized_host.py compiles it on its
// own.  The pass split is sized_geom.hpp's (split_passes), counted in groups.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sized_geom.hpp"

namespace uplink_ec {
namespace b3list {

constexpr uint64_t kChunkBytes = 1024;  // a BLAKE3 chunk
constexpr uint64_t kGroupChunks = 256;  // chunks one workgroup folds (blake3_device.hpp kGroup)
constexpr uint64_t kMaxGroups = 256;    // groups one parents workgroup folds: pieces up to 64 MiB
// a pass's staging is bounded by its pieces (a 64-byte record each) and by its
// workgroups (4 bytes of map and at most 32 bytes of node scratch each)
constexpr size_t kPassPieces = 16384;
constexpr int64_t kPassGroups = (int64_t)1 << 18;

// an empty piece is one (empty) chunk
inline uint64_t chunks_of(uint64_t len) { return len ? (len - 1) / kChunkBytes + 1 : 1; }
inline uint64_t groups_of(uint64_t len) { return (chunks_of(len) - 1) / kGroupChunks + 1; }
// subtree CVs a piece leaves for the parents kernel: none when one group finishes it
inline uint64_t node_slots(uint64_t len) { return groups_of(len) > 1 ? groups_of(len) : 0; }

// Byte t of a piece is at base + (t / run)*run_stride + t % run (run == 0, run >=
// len or run_stride == run: contiguous).
struct Piece {
    uint64_t base;  // device address
    uint64_t len;
    uint64_t run;
    int64_t run_stride;
};

// The piece's run as the kernels take it (blake3.hip normalized()): a contiguous
// piece is one run of 2^62 bytes; run_shift = log2(run) for a power of two, else -1.
struct Run {
    uint64_t run;
    int64_t run_stride;
    int32_t run_shift;
};

inline Run run_of(const Piece &p) {
    Run r{p.run, p.run_stride, -1};
    if (r.run == 0 || r.run >= p.len || r.run_stride == (int64_t)r.run) {
        r.run = 1ull << 62;
        r.run_stride = 0;
    }
    if ((r.run & (r.run - 1)) == 0) {
        int32_t s = 0;
        while ((r.run >> s) != 1) s++;
        r.run_shift = s;
    }
    return r;
}

enum Class : uint8_t {
    kFast = 0,      // 16-byte loads: runs of a power of two >= 64 bytes, base and run stride 16-byte aligned
    kByte = 1,      // byte loads: anything else
    kOversize = 2,  // more than kMaxGroups groups: on its own through the uniform launch
};

inline Class classify(const Piece &p) {
    if (groups_of(p.len) > kMaxGroups) return kOversize;
    const Run r = run_of(p);
    return r.run_shift >= 6 && (p.base & 15) == 0 && (r.run_stride & 15) == 0 ? kFast : kByte;
}

// A pass laid out.  Pieces of class kOversize take no part (their entries stay 0
// / kNone).  The fast pieces' workgroups are one launch, the byte pieces' another,
// each numbered from 0; `map` holds the fast launch's entries, then the byte
// launch's: map[first(cls) + w] = position of the piece workgroup w of that
// launch works on.
constexpr uint32_t kNone = 0xFFFFFFFFu;
struct Layout {
    std::vector<uint32_t> wg0;     // [piece] its first workgroup in its class's launch
    std::vector<uint32_t> node0;   // [piece] its first node slot (pieces of >= 2 groups)
    std::vector<uint32_t> groups;  // [piece]
    std::vector<uint32_t> map;
    std::vector<uint32_t> parents;  // positions of the pieces of 2..kMaxGroups groups: one parents workgroup each
    uint32_t wgs[2] = {0, 0};       // workgroups of the fast and of the byte launch
    uint32_t nodes = 0;             // node slots of the pass
    uint32_t first(Class c) const { return c == kFast ? 0 : wgs[0]; }
};

// pieces[0..n) with their classes; n <= kPassPieces and at most kPassGroups groups
// (plus one piece's), so every count fits 32 bits.
inline Layout layout(const Piece *pieces, const Class *cls, size_t n) {
    Layout L;
    L.wg0.assign(n, 0);
    L.node0.assign(n, kNone);
    L.groups.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (cls[i] == kOversize) continue;
        const uint32_t g = (uint32_t)groups_of(pieces[i].len);
        L.groups[i] = g;
        L.wg0[i] = L.wgs[cls[i]];
        L.wgs[cls[i]] += g;
        if (g > 1) {
            L.node0[i] = L.nodes;
            L.nodes += g;
            L.parents.push_back((uint32_t)i);
        }
    }
    L.map.assign((size_t)L.wgs[0] + L.wgs[1], kNone);
    for (size_t i = 0; i < n; i++) {
        if (cls[i] == kOversize) continue;
        uint32_t *m = L.map.data() + L.first(cls[i]) + L.wg0[i];
        for (uint32_t g = 0; g < L.groups[i]; g++) m[g] = (uint32_t)i;
    }
    return L;
}

// The passes of a list: consecutive pieces, at most max_pieces of them and
// max_groups workgroups per pass (an oversize piece counts no workgroup: it is
// not in the pass's launches).
inline std::vector<sized::Pass> split(const Piece *pieces, const Class *cls, size_t n, size_t max_pieces = kPassPieces,
                                      int64_t max_groups = kPassGroups) {
    std::vector<int64_t> g(n);
    for (size_t i = 0; i < n; i++) g[i] = cls[i] == kOversize ? 0 : (int64_t)groups_of(pieces[i].len);
    return sized::split_passes(g.data(), n, max_pieces, max_groups);
}

}  // namespace b3list
}  // namespace uplink_ec
