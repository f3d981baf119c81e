// Geometry of an encode call whose segments differ in size (include/uplink_ec.h
// ec_encode_segments_sized, rs_encode_sized.hpp): the compile-time encoder's
// 1-KiB column blocks per segment, each segment's first block among the blocks
// of a pass, the pass's tiles (pairs of blocks), and PadReader's padding with
// the check that a segment's stripe count is the one its data length pads to.
// Plain C++, no HIP: tests/test_encode_sized_host.py compiles it on its own.
// The 32-bit chunk limit and the passes a call is cut into are sized_geom.hpp's
// (chunks_of, split_passes), counted in blocks here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sized_geom.hpp"

namespace uplink_ec {
namespace sized {

constexpr int64_t kBlockChunks = 64;  // 16-byte chunks of one share row per block (rs_tile.hpp block_cols)

inline int64_t blocks_of(int64_t chunks) { return (chunks + kBlockChunks - 1) / kBlockChunks; }

// block0[i] = the first block of segment i among the blocks of segments 0 .. n-1
// concatenated; returns their total.
inline int64_t first_blocks(const int64_t *blocks, size_t n, int64_t *block0) {
    int64_t b = 0;
    for (size_t i = 0; i < n; i++) {
        block0[i] = b;
        b += blocks[i];
    }
    return b;
}

// Tiles of a pass of B blocks: tile t is block t and block t + pair_count(B)
// (rs_tile.hpp pair_cols); with B odd the last tile has no second block.
inline int64_t pair_count(int64_t total_blocks) { return (total_blocks + 1) >> 1; }

// Bytes PadReader appends to data_len bytes for stripes of `stripe` bytes
// (encryption.PadReader, single.go:233-238: at least 4, the last 4 their count):
// what ec_pad_segments writes.  0 when the sum does not fit 64 bits.
inline uint64_t pad_amount(uint64_t data_len, uint64_t stripe) {
    if (stripe == 0 || data_len > UINT64_MAX - 4 - stripe) return 0;
    return 4 + (stripe - (data_len + 4) % stripe) % stripe;
}

// nstripes stripes are exactly data_len bytes and their padding.
inline bool pad_matches(uint64_t data_len, uint64_t nstripes, uint64_t stripe) {
    const uint64_t p = pad_amount(data_len, stripe);
    if (p == 0 || nstripes > UINT64_MAX / stripe) return false;
    return nstripes * stripe == data_len + p;
}

}  // namespace sized
}  // namespace uplink_ec
