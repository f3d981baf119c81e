// Geometry of a ranged download (include/uplink_ec.h ec_gcm_open_ranges_sized;
// uplink_amd/downloads.py range_geometry): what a plaintext range
// [off, off+len) of a segment costs at every layer of the reference.
// decryptRanger's Range (streams/store.go:347-382, encryption.Transform) asks for
// the cipher blocks CalcEncompassingBlocks(off, len, in_block) gives, opens block
// b under nonce + b, discards the head of the first block and limits the length;
// decodedRanger.Range (eestream/decode.go:199-227) does the same one level down
// with the stripes that cover those blocks' encrypted bytes.  Plain C++, no HIP:
// tests/test_ranges_host.py compiles it on its own.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uplink_ec {
namespace rangegeom {

constexpr uint64_t kTagBytes = 16;
constexpr uint64_t kMaxInBlock = 1u << 24;     // the cipher's rule (gcm_launch_sized)
constexpr uint64_t kMaxBlockEnd = 0x7FFFFFFFu;  // first block + blocks (status words are int32)

// encryption.CalcEncompassingBlocks: the blocks of block_size bytes that cover
// [off, off+len); a length of 0 gives a count of 0.  block_size > 0 and off + len
// fits 64 bits (the callers below ensure both).
struct Blocks {
    uint64_t first, count;
};
inline Blocks encompassing_blocks(uint64_t off, uint64_t len, uint64_t block_size) {
    const uint64_t first = off / block_size;
    if (len == 0) return {first, 0};
    const uint64_t end = off + len, last = end / block_size;
    return {first, last - first + (end % block_size ? 1 : 0)};
}

enum : int { kOk = 0, kInvalid = 1, kUnsupported = 2 };

// Plaintext range (off, len) of a segment of plain_size bytes, encrypted in blocks
// of block_size bytes (in_block = block_size - 16 of plaintext each) and erasure
// coded with k shares of ess bytes per stripe.  err != 0 leaves every other field 0.
struct RangeGeom {
    int err;                   // kInvalid: outside [0, plain_size], a bad shape or 64-bit overflow;
                               // kUnsupported: first_block + nblocks above 0x7FFFFFFF
    uint64_t first_block, nblocks, head;  // covered blocks fb .. fb+nb-1; the range starts head bytes into block fb
    uint64_t enc_off, enc_len;            // their encrypted bytes: fb*B, nb*B
    uint64_t first_stripe, nstripes, skip;  // covering stripes; the blocks start skip bytes into the decoded stripes
    uint64_t piece_off, piece_len;        // what every piece contributes: [fs*ess, (fs+ns)*ess)
};

inline RangeGeom range_geometry(uint64_t plain_size, uint64_t off, uint64_t len, uint64_t block_size, uint64_t k,
                                uint64_t ess) {
    RangeGeom bad{kInvalid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (block_size <= kTagBytes || k == 0 || ess == 0) return bad;
    const uint64_t ib = block_size - kTagBytes;
    if (ib % 16 || ib > kMaxInBlock) return bad;
    if (off > plain_size || len > plain_size - off) return bad;
    uint64_t S;
    if (__builtin_mul_overflow(k, ess, &S)) return bad;
    RangeGeom g{kOk, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const Blocks b = encompassing_blocks(off, len, ib);
    if (b.first + b.count > kMaxBlockEnd) {
        bad.err = kUnsupported;
        return bad;
    }
    g.first_block = b.first, g.nblocks = b.count, g.head = off - b.first * ib;
    g.enc_off = b.first * block_size, g.enc_len = b.count * block_size;  // below 2^31 * (2^24 + 16)
    const Blocks s = encompassing_blocks(g.enc_off, g.enc_len, S);
    g.first_stripe = s.first, g.nstripes = s.count, g.skip = g.enc_off - s.first * S;
    uint64_t end;  // (fs + ns) * S may pass 64 bits for an absurd stripe: refuse it
    if (__builtin_mul_overflow(s.first + s.count, S, &end)) return bad;
    g.piece_off = s.first * ess, g.piece_len = s.count * ess;
    return g;
}

// What ec_gcm_open_ranges_sized requires of a segment: the range starts inside its
// first covered block and nblocks is exactly the count that covers it.
inline bool covers(uint64_t head, uint64_t len, uint64_t in_block, uint64_t nblocks) {
    if (in_block == 0 || head >= in_block || len > UINT64_MAX - head) return false;
    return encompassing_blocks(head, len, in_block).count == nblocks;
}

}  // namespace rangegeom
}  // namespace uplink_ec
