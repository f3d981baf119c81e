// Geometry of an AES-256-GCM call over segments that each have their own number
// of blocks (include/uplink_ec.h ec_gcm_seal_segments_sized /
// ec_gcm_open_segments_sized; kernel gcm_blocks_sized in aesgcm.hip): the
// workgroups each segment of a pass gets, each segment's first workgroup, the
// workgroup -> segment map, the passes a long list is cut into, PadReader's
// padding to the cipher's block with the check that a segment's block count is
// the one its data length pads to, and the sizes of an upload through the cipher.
// Plain C++, no HIP: tests/test_gcm_sized_host.py compiles it on its own.  The
// pass split is sized_geom.hpp's (split_passes), the padding rule
// enc_sized_geom.hpp's (pad_amount, pad_matches) with in_block for the stripe.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "enc_sized_geom.hpp"
#include "sized_geom.hpp"

namespace uplink_ec {
namespace gcmsized {

constexpr uint32_t kWaves = 4;          // waves of a workgroup: one GCM block each per iteration (aesgcm.hip)
constexpr size_t kPassSegs = 4096;      // segments of a pass: 48 bytes of staging and 32 of descriptor each
constexpr uint64_t kMaxBlocks = 0x7FFFFFFFu;  // blocks of one segment (status words are int32)
constexpr uint32_t kTagBytes = 16;

// Workgroups of a segment of nblocks blocks in a pass of total_blocks, T the grid
// the uniform launch aims for: its share of T in proportion to its blocks, at
// least one, and never more than give every wave a block.  A small pass gives
// every wave at most one block; a pass larger than the chip shares T workgroups,
// whose waves then loop.  0 for a skipped segment.
inline uint32_t wgs_of(uint64_t nblocks, uint64_t total_blocks, uint32_t T) {
    if (nblocks == 0) return 0;
    const uint64_t full = (nblocks + kWaves - 1) / kWaves;
    uint64_t share = total_blocks ? (nblocks * T + total_blocks - 1) / total_blocks : 1;  // nblocks < 2^31, T <= 2^14
    if (share < 1) share = 1;
    return (uint32_t)(full < share ? full : share);
}

// A pass laid out.
struct Layout {
    std::vector<uint32_t> wg0;  // [segment] its first workgroup
    std::vector<uint32_t> wgs;  // [segment] its workgroups (0: skipped)
    std::vector<uint32_t> map;  // [workgroup] -> segment
    uint64_t total_blocks = 0;
};

// nblocks[0..n), n <= kPassSegs and every count <= kMaxBlocks: the grid is at most T + n.
inline Layout layout(const uint64_t *nblocks, size_t n, uint32_t T) {
    Layout L;
    L.wg0.assign(n, 0);
    L.wgs.assign(n, 0);
    for (size_t i = 0; i < n; i++) L.total_blocks += nblocks[i];
    uint32_t w = 0;
    for (size_t i = 0; i < n; i++) {
        L.wg0[i] = w;
        L.wgs[i] = wgs_of(nblocks[i], L.total_blocks, T);
        w += L.wgs[i];
    }
    L.map.resize(w);
    for (size_t i = 0; i < n; i++)
        for (uint32_t g = 0; g < L.wgs[i]; g++) L.map[L.wg0[i] + g] = (uint32_t)i;
    return L;
}

// The blocks wave `wave` of workgroup `wg` (of the segment's wgs) takes, in order:
// the kernel's stride loop.
template <class F>
inline void for_blocks(uint32_t wg, uint32_t wave, uint32_t wgs, uint32_t nblocks, F &&f) {
    for (uint32_t b = wg * kWaves + wave; b < nblocks; b += wgs * kWaves) f(b);
}

// The passes of a list of n segments: consecutive segments, at most max_segs each.
inline std::vector<sized::Pass> split(size_t n, size_t max_segs = kPassSegs) {
    const std::vector<int64_t> one(n, 1);
    return sized::split_passes(one.data(), n, max_segs, INT64_MAX);
}

// nblocks blocks of in_block bytes are exactly data_len bytes and PadReader's padding.
inline bool pad_matches(uint64_t data_len, uint64_t nblocks, uint64_t in_block) {
    return sized::pad_matches(data_len, nblocks, in_block);
}
inline uint64_t pad_amount(uint64_t data_len, uint64_t in_block) { return sized::pad_amount(data_len, in_block); }

// An upload of `size` bytes through TransformWriterPadded for blocks of in_block
// plaintext bytes: its blocks, the bytes its padded plaintext takes and the bytes
// of its ciphertext.  All 0 when a size does not fit 64 bits.
struct CipherSizes {
    uint64_t nblocks, plain_cap, enc_len;
};
inline CipherSizes cipher_sizes(uint64_t size, uint64_t in_block) {
    const uint64_t p = sized::pad_amount(size, in_block);
    if (p == 0) return {0, 0, 0};
    const uint64_t cap = size + p, nb = cap / in_block;
    if (nb > (UINT64_MAX - cap) / kTagBytes) return {0, 0, 0};
    return {nb, cap, cap + nb * kTagBytes};
}

}  // namespace gcmsized
}  // namespace uplink_ec
