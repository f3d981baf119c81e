// SHA-256 primitives shared by the piece-hash kernel (sha256.hip) and the host
// test (tests/c/sha_list_geom_test.cpp): the compression function of FIPS 180-4
// §6.2.2 over a 16-word schedule ring, and the builder of a message's last one
// or two blocks (§5.1.1).  Plain C++: the host compiler takes this header on its
// own, with the function markers defined away, and runs the very same rounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UPLINK_SHA_HD __host__ __device__ __forceinline__
#else
#define UPLINK_SHA_HD inline
#endif

namespace uplink_ec {
namespace sha256 {

constexpr uint32_t kInit[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                               0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};

// (every index is a constant once the rounds are unrolled: the values become immediates)
constexpr uint32_t kK[64] = {
    0x428A2F98u, 0x71374491u, 0xB5C0FBCFu, 0xE9B5DBA5u, 0x3956C25Bu, 0x59F111F1u, 0x923F82A4u, 0xAB1C5ED5u,
    0xD807AA98u, 0x12835B01u, 0x243185BEu, 0x550C7DC3u, 0x72BE5D74u, 0x80DEB1FEu, 0x9BDC06A7u, 0xC19BF174u,
    0xE49B69C1u, 0xEFBE4786u, 0x0FC19DC6u, 0x240CA1CCu, 0x2DE92C6Fu, 0x4A7484AAu, 0x5CB0A9DCu, 0x76F988DAu,
    0x983E5152u, 0xA831C66Du, 0xB00327C8u, 0xBF597FC7u, 0xC6E00BF3u, 0xD5A79147u, 0x06CA6351u, 0x14292967u,
    0x27B70A85u, 0x2E1B2138u, 0x4D2C6DFCu, 0x53380D13u, 0x650A7354u, 0x766A0ABBu, 0x81C2C92Eu, 0x92722C85u,
    0xA2BFE8A1u, 0xA81A664Bu, 0xC24B8B70u, 0xC76C51A3u, 0xD192E819u, 0xD6990624u, 0xF40E3585u, 0x106AA070u,
    0x19A4C116u, 0x1E376C08u, 0x2748774Cu, 0x34B0BCB5u, 0x391C0CB3u, 0x4ED8AA4Au, 0x5B9CCA4Fu, 0x682E6FF3u,
    0x748F82EEu, 0x78A5636Fu, 0x84C87814u, 0x8CC70208u, 0x90BEFFFAu, 0xA4506CEBu, 0xBEF9A3F7u, 0xC67178F2u};

UPLINK_SHA_HD uint32_t rotr(uint32_t x, int n) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateright32)
    return __builtin_rotateright32(x, (uint32_t)n);
#else
    return (x >> n) | (x << (32 - n));
#endif
#else
    return (x >> n) | (x << (32 - n));
#endif
}

// a ^ b ^ c.  Written plainly the compiler emits two v_xor_b32 for it on gfx950 (it does pick
// v_alignbit_b32 for the rotates, v_bitop3_b32 for Ch and Maj and v_add3_u32 for the sums), so
// the device side names the one-instruction form: v_bitop3_b32 with truth table 0x96.
UPLINK_SHA_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// h <- compress(h, w): w holds the block's sixteen words, most significant byte
// first, and is used up as the schedule's ring (W[t] lives in w[t % 16]).
UPLINK_SHA_HD void compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma GCC unroll 64
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
            w[t & 15] += xor3(rotr(x, 7), rotr(x, 18), x >> 3) + w[(t - 7) & 15] + xor3(rotr(y, 17), rotr(y, 19), y >> 10);
        }
        const uint32_t t1 = hh + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK[t] + w[t & 15];
        const uint32_t t2 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}

// blocks of a message of len bytes, padding included (len < 2^61: its bit count fits 64 bits)
UPLINK_SHA_HD uint64_t blocks_of(uint64_t len) { return (len + 8) / 64 + 1; }

// The padding of block `blk` of a message of len bytes.  On entry w holds the
// block's message bytes as words (most significant byte first) with zeros where
// the message has none.  The 0x80 goes behind the last message byte where that
// position lies in this block, and the message's bit count, most significant
// word first, into the last two words of the message's last block.
UPLINK_SHA_HD void pad_block(uint32_t (&w)[16], uint64_t len, uint64_t blk) {
    if (len / 64 == blk) {
        const uint32_t r = (uint32_t)(len % 64);
#pragma GCC unroll 16
        for (int i = 0; i < 16; i++)
            if ((uint32_t)i == r / 4) w[i] |= 0x80000000u >> (8 * (r % 4));
    }
    if (blk + 1 == blocks_of(len)) {
        w[14] = (uint32_t)(len >> 29);
        w[15] = (uint32_t)(len << 3);
    }
}

UPLINK_SHA_HD uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

}  // namespace sha256
}  // namespace uplink_ec
