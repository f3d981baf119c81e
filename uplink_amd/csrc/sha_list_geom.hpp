// Geometry of a SHA-256 call over a list of pieces that each have their own
// length (include/uplink_ec.h ec_sha256_pieces_list, ec_sha256_segments_sized;
// kernel in sha256.hip): blocks per piece, the fast / byte classes, the lane
// order of a pass with its lane -> row map, the passes of a long list and the
// launches a pass takes.  Plain C++, no HIP: tests/test_sha256_host.py compiles
// it on its own.  Pieces and their runs are b3_list_geom.hpp's (Piece, run_of),
// the pass split is sized_geom.hpp's (split_passes).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "b3_list_geom.hpp"

namespace uplink_ec {
namespace shalist {

using b3list::Piece;
using b3list::run_of;
using b3list::kNone;
using b3list::kPassPieces;

constexpr uint64_t kBlockBytes = 64;
constexpr uint64_t kMaxLen = (1ull << 61) - 1;  // the bit count of a message fits 64 bits
constexpr uint32_t kWave = 64;                  // lanes per workgroup: one wave, one class
// blocks a launch advances every piece by at most (1 MiB per piece): keeps each
// kernel short whatever the longest piece is; the state is carried between launches
constexpr uint64_t kLaunchBlocks = 16384;

// 64-byte blocks of a piece, padding included (0x80 and the 8-byte bit count)
inline uint64_t blocks_of(uint64_t len) { return (len + 8) / kBlockBytes + 1; }

enum Class : uint8_t {
    kFast = 0,  // 16-byte loads: contiguous or runs of a power of two >= 64 bytes, base and run stride 16-byte aligned
    kByte = 1,  // byte loads: anything else
};

inline Class class_of(const Piece &p) {
    const b3list::Run r = run_of(p);
    return r.run_shift >= 6 && (p.base & 15) == 0 && (r.run_stride & 15) == 0 ? kFast : kByte;
}

// A pass laid out: one lane per piece.  The fast pieces come first, then the
// byte pieces, each class by block count in descending order (ties in list
// order) so that the lanes of a wave retire together, and each class padded to
// whole waves so that no wave mixes classes.
struct Layout {
    std::vector<uint32_t> row;  // [lane] position of its piece in the pass, kNone: a padding lane
    uint32_t count[2] = {0, 0};  // pieces of the fast and of the byte class
    uint64_t max_blocks = 0;     // of the longest piece
    uint32_t lanes() const { return (uint32_t)row.size(); }
    uint32_t waves() const { return lanes() / kWave; }
};

// pieces[0..n), n <= kPassPieces
inline Layout layout(const Piece *pieces, size_t n) {
    Layout L;
    std::vector<uint32_t> idx[2];
    for (size_t i = 0; i < n; i++) {
        idx[class_of(pieces[i])].push_back((uint32_t)i);
        L.max_blocks = std::max(L.max_blocks, blocks_of(pieces[i].len));
    }
    for (int c = 0; c < 2; c++) {
        std::stable_sort(idx[c].begin(), idx[c].end(),
                         [&](uint32_t x, uint32_t y) { return blocks_of(pieces[x].len) > blocks_of(pieces[y].len); });
        L.count[c] = (uint32_t)idx[c].size();
        L.row.insert(L.row.end(), idx[c].begin(), idx[c].end());
        L.row.resize((L.row.size() + kWave - 1) / kWave * kWave, kNone);
    }
    return L;
}

// The passes of a list: consecutive pieces, at most max_pieces per pass.
inline std::vector<sized::Pass> split(size_t n, size_t max_pieces = kPassPieces) {
    const std::vector<int64_t> none(n, 0);
    return sized::split_passes(none.data(), n, max_pieces, 0);
}

// Launches that take a piece of max_blocks blocks to its digest at launch_blocks per launch.
inline uint64_t launches_of(uint64_t max_blocks, uint64_t launch_blocks = kLaunchBlocks) {
    return max_blocks ? (max_blocks - 1) / launch_blocks + 1 : 0;
}

}  // namespace shalist
}  // namespace uplink_ec
