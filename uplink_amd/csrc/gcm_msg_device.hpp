// Arithmetic of the one-shot message cipher (kernel gcm_messages in aesgcm.hip;
// include/uplink_ec.h ec_gcm_seal_messages / ec_gcm_open_messages) as plain C++
// that compiles for the host and for the device: the AES-256 key expansion from
// the 32 key bytes, the GF(2^128) multiply in its two forms (bit by bit, and on a
// 4-bit table of the multiplier), a lane's Horner run, the combination of the 64
// lanes' partial sums, and the builders of the counter blocks, the length block
// and the message's short last slot.  tests/c/gcm_msg_host_test.cpp includes
// this file alone, plays the 64 lanes in a loop and is checked against the GCM
// specification's vectors and the CPU oracle without a GPU.
//
// The GHASH of a message, front padded to 64 * R slots Y[0 .. 64R) (gcm_msg_geom.hpp):
// lane l runs Horner over its R slots with multiplier H,
//     P_l = sum_j Y[l*R + j] * H^(R - j),
// and the GHASH is sum_l P_l * H^(R * (63 - l)).  That sum is taken pairwise: at
// distance d = 1, 2, 4, .. 32 lane l and lane l ^ d both get
//     (the lower lane's value) * M_d + (the upper lane's value),  M_d = H^(R * d),
// M_2d = M_d * M_d.  Every multiplier (H, M_d) is the same for all lanes of the
// message's wave, which is what lets the wave keep it in scalar registers or build
// one table of it.  After the last step every lane holds the GHASH.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UPLINK_HD __host__ __device__ inline
#else
#define UPLINK_HD inline
#endif
#if defined(__clang__)
#define UPLINK_UNROLL _Pragma("unroll")
#define UPLINK_UNROLL8 _Pragma("unroll 8")
#define UPLINK_NOUNROLL _Pragma("unroll 1")
#else
#define UPLINK_UNROLL
#define UPLINK_UNROLL8
#define UPLINK_NOUNROLL
#endif

namespace uplink_ec {
namespace gcmmsg {

// A 16-byte block as four big-endian words: w[0] holds bytes 0..3, byte 0 on top.
struct Block {
    uint32_t w[4];
};
UPLINK_HD Block operator^(const Block &a, const Block &b) {
    return {{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}};
}
UPLINK_HD bool operator==(const Block &a, const Block &b) {
    return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) == 0;
}
UPLINK_HD Block zero_block() { return {{0, 0, 0, 0}}; }

UPLINK_HD uint32_t load_be32(const uint8_t *p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}
UPLINK_HD uint8_t block_byte(const Block &b, uint32_t i) { return (uint8_t)(b.w[i >> 2] >> (24 - 8 * (i & 3))); }

// ---- AES-256 key expansion; sbox(x): the S-box of byte x ----

template <class Sbox>
UPLINK_HD uint32_t sub_word(uint32_t w, Sbox sbox) {
    return (uint32_t)sbox(w >> 24) << 24 | (uint32_t)sbox((w >> 16) & 255) << 16 | (uint32_t)sbox((w >> 8) & 255) << 8 |
           (uint32_t)sbox(w & 255);
}

// kw: the key as eight big-endian words.  Straight-line once unrolled: no round
// key is ever indexed by a run-time value, so rk stays in registers.
template <class Sbox>
UPLINK_HD void key_expand(const uint32_t (&kw)[8], uint32_t (&rk)[60], Sbox sbox) {
UPLINK_UNROLL
    for (int i = 0; i < 8; i++) rk[i] = kw[i];
    uint32_t rcon = 1;
UPLINK_UNROLL
    for (int i = 8; i < 60; i++) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = sub_word((t << 8) | (t >> 24), sbox) ^ (rcon << 24);
            rcon = (rcon << 1) ^ ((rcon & 0x80) ? 0x11b : 0);
        } else if (i % 8 == 4) {
            t = sub_word(t, sbox);
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

// AES-256 of one block from the S-box alone (the host's and the tests'; the
// kernel runs the file's T-table rounds on the same round keys)
UPLINK_HD uint32_t xtime32(uint32_t a) { return ((a << 1) ^ ((a & 0x80) ? 0x1b : 0)) & 0xff; }
template <class Sbox>
UPLINK_HD Block aes256_encrypt(const Block &in, const uint32_t (&rk)[60], Sbox sbox) {
    uint32_t s[4];
    for (int i = 0; i < 4; i++) s[i] = in.w[i] ^ rk[i];
    for (int r = 1; r <= 14; r++) {
        uint32_t t[4];
        for (int i = 0; i < 4; i++) {
            // SubBytes + ShiftRows: column i takes row j from column i + j
            const uint32_t c0 = sbox(s[i] >> 24), c1 = sbox((s[(i + 1) & 3] >> 16) & 255),
                           c2 = sbox((s[(i + 2) & 3] >> 8) & 255), c3 = sbox(s[(i + 3) & 3] & 255);
            uint32_t m0 = c0, m1 = c1, m2 = c2, m3 = c3;
            if (r != 14) {  // MixColumns
                m0 = xtime32(c0) ^ xtime32(c1) ^ c1 ^ c2 ^ c3;
                m1 = c0 ^ xtime32(c1) ^ xtime32(c2) ^ c2 ^ c3;
                m2 = c0 ^ c1 ^ xtime32(c2) ^ xtime32(c3) ^ c3;
                m3 = xtime32(c0) ^ c0 ^ c1 ^ c2 ^ xtime32(c3);
            }
            t[i] = (m0 << 24 | m1 << 16 | m2 << 8 | m3) ^ rk[4 * r + i];
        }
        for (int i = 0; i < 4; i++) s[i] = t[i];
    }
    return {{s[0], s[1], s[2], s[3]}};
}

// ---- GF(2^128), GCM bit order: bit 31 of w[0] is the coefficient of x^0 ----

// v * x: one right shift, the bit shifted out folded back through
// x^128 = x^7 + x^2 + x + 1
UPLINK_HD Block gf_times_x(const Block &v) {
    const uint32_t carry = v.w[3] & 1;
    return {{(v.w[0] >> 1) ^ (carry ? 0xE1000000u : 0), (v.w[1] >> 1) | (v.w[0] << 31), (v.w[2] >> 1) | (v.w[1] << 31),
             (v.w[3] >> 1) | (v.w[2] << 31)}};
}

// x * m bit by bit (the specification's Algorithm 1).  The run of m * x^i does not
// depend on x: with m the same for a whole wave it is scalar work.
UPLINK_HD Block gf_mul_bits(const Block &x, const Block &m) {
    Block z = zero_block(), v = m;
UPLINK_UNROLL
    for (int q = 0; q < 4; q++) {
UPLINK_UNROLL8
        for (int i = 31; i >= 0; i--) {
            const uint32_t mask = 0u - ((x.w[q] >> i) & 1);
            z.w[0] ^= v.w[0] & mask, z.w[1] ^= v.w[1] & mask, z.w[2] ^= v.w[2] & mask, z.w[3] ^= v.w[3] & mask;
            v = gf_times_x(v);
        }
    }
    return z;
}

// Entry n of Shoup's 4-bit table of m: n * m, bit 3 of n the coefficient of x^0.
UPLINK_HD Block gf_table_entry(const Block &m, uint32_t n) {
    Block z = zero_block(), v = m;
UPLINK_UNROLL
    for (int b = 3; b >= 0; b--) {
        const uint32_t mask = 0u - ((n >> b) & 1);
        z.w[0] ^= v.w[0] & mask, z.w[1] ^= v.w[1] & mask, z.w[2] ^= v.w[2] & mask, z.w[3] ^= v.w[3] & mask;
        v = gf_times_x(v);
    }
    return z;
}

// What the four bits shifted out of a product by x^4 fold back to, at the top of
// w[0]: n carry-less times 0x1C20 (0xE1 shifted through the four positions).
UPLINK_HD uint32_t gf_rem4(uint32_t n) { return ((n << 5) ^ (n << 10) ^ (n << 11) ^ (n << 12)) << 16; }

// x * m on m's 4-bit table tab[16] (gf_table_entry): Horner over x's 32 nibbles
// from the last, a shift by x^4 and one lookup each.  The words of x are taken
// from the last in a loop that is kept a loop (the eight nibbles of a word
// unrolled inside it): unrolled whole, the 32 lookups of a product are all in
// flight at once and the kernel runs out of registers.
template <class Tab>
UPLINK_HD Block gf_mul_table(const Block &x, Tab tab) {
    uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
    uint32_t x0 = x.w[0], x1 = x.w[1], x2 = x.w[2], x3 = x.w[3];
UPLINK_NOUNROLL
    for (int q = 0; q < 4; q++) {
        const uint32_t w = x3;
        x3 = x2, x2 = x1, x1 = x0;
UPLINK_UNROLL
        for (int k = 0; k < 8; k++) {
            const uint32_t r = gf_rem4(z3 & 15);  // (nothing to shift out before the first nibble: z is 0)
            z3 = (z3 >> 4) | (z2 << 28);
            z2 = (z2 >> 4) | (z1 << 28);
            z1 = (z1 >> 4) | (z0 << 28);
            z0 = (z0 >> 4) ^ r;
            const Block t = tab((w >> (4 * k)) & 15);
            z0 ^= t.w[0], z1 ^= t.w[1], z2 ^= t.w[2], z3 ^= t.w[3];
        }
    }
    return {{z0, z1, z2, z3}};
}

// The two forms of "multiply by the wave's current multiplier".  set(m) makes m
// the multiplier, mul(x) is x * m.  The table form here fills its 16 entries in a
// loop; the kernel's (aesgcm.hip MsgMulTable) lets 16 lanes fill one each into
// LDS and otherwise runs the same gf_table_entry and gf_mul_table.
struct MulBits {
    Block m;
    UPLINK_HD void set(const Block &x) { m = x; }
    UPLINK_HD Block mul(const Block &x) const { return gf_mul_bits(x, m); }
};
struct MulTable {
    Block tab[16];
    UPLINK_HD void set(const Block &x) {
        for (uint32_t n = 0; n < 16; n++) tab[n] = gf_table_entry(x, n);
    }
    UPLINK_HD Block mul(const Block &x) const {
        const Block *t = tab;
        return gf_mul_table(x, [t](uint32_t n) { return t[n]; });
    }
};

// One Horner step of a lane: (acc + y) * H, mul the multiply by H.
template <class Mul>
UPLINK_HD Block horner_step(const Block &acc, const Block &y, const Mul &mul) {
    return mul.mul(acc ^ y);
}

// One step of the pairwise combination, for one lane: `mine` its value,
// `partner` that of lane ^ d, upper = the lane has bit d set, mul the multiply by
// M_d.  Both lanes of a pair get the same result.
template <class Mul>
UPLINK_HD Block combine_step(const Block &mine, const Block &partner, bool upper, const Mul &mul) {
    const Block lo = upper ? partner : mine, hi = upper ? mine : partner;
    return mul.mul(lo) ^ hi;
}

// The combination as a function of the 64 lanes' partial sums: `steps` steps
// (gcm_msg_geom.hpp combine_steps; 6 for a message that fills the wave) starting
// from M_1 = hr = H^R.  Returns lane 63's value, the GHASH.  The kernel runs the
// same steps with the partner's value taken by a cross-lane shuffle.
template <class Mul>
UPLINK_HD Block combine64(const Block (&partial)[64], const Block &hr, uint32_t steps, Mul &mul) {
    Block cur[64], next[64];
    for (int l = 0; l < 64; l++) cur[l] = partial[l];
    Block m = hr;
    for (uint32_t s = 0; s < steps; s++) {
        const uint32_t d = 1u << s;
        mul.set(m);
        for (uint32_t l = 0; l < 64; l++) next[l] = combine_step(cur[l], cur[l ^ d], (l & d) != 0, mul);
        for (int l = 0; l < 64; l++) cur[l] = next[l];
        m = mul.mul(m);  // M_2d = M_d^2
    }
    return cur[63];
}

// ---- the blocks GCM builds around a message ----

// nonce (12 bytes) || ctr: J0 is ctr 1, ciphertext slot i is ctr 2 + i.
// nw: the nonce as three big-endian words.
UPLINK_HD Block counter_block(const uint32_t (&nw)[3], uint32_t ctr) { return {{nw[0], nw[1], nw[2], ctr}}; }

// len(A) = 0 || len(C), both in bits
UPLINK_HD Block length_block(uint64_t len_bytes) {
    const uint64_t bits = len_bytes * 8;
    return {{0, 0, (uint32_t)(bits >> 32), (uint32_t)bits}};
}

// the first n bytes (n <= 16) of b, the rest zero: GHASH sees the message's
// short last slot zero padded
UPLINK_HD Block keep_bytes(const Block &b, uint32_t n) {
    Block r;
UPLINK_UNROLL
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t lo = 4 * q;
        r.w[q] = b.w[q] & (n >= lo + 4 ? 0xffffffffu : n <= lo ? 0u : ~(0xffffffffu >> (8 * (n - lo))));
    }
    return r;
}

// n bytes (n <= 16) at p as a zero-padded block
UPLINK_HD Block load_bytes(const uint8_t *p, uint32_t n) {
    Block r = zero_block();
    for (uint32_t i = 0; i < n; i++) r.w[i >> 2] |= (uint32_t)p[i] << (24 - 8 * (i & 3));
    return r;
}

}  // namespace gcmmsg
}  // namespace uplink_ec
