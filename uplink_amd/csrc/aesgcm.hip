// AES-256-GCM segment encryption and decryption on the GPU (SURVEY.md §8f
// row 4).
//
// Replaces, for whole segments, what the upload's splitter does through
// encryption.TransformWriterPadded(buf, NewEncrypter(EncAESGCM, &contentKey,
// &nonce, BlockSize)) (private/storage/streams/splitter/splitter.go:156,170)
// and what the download does through decryptRanger (streams/store.go:347-382):
// AES-256-GCM over blocks of InBlockSize = BlockSize - 16 plaintext bytes,
// block b sealed under nonce + b (12 bytes, little-endian increment),
// written as ciphertext || tag.  BlockSize is 29*256 (project.go:84), so an
// encrypted block is exactly one RS(29,80) stripe.  The cipher code is
// storj.io/common/encryption (go.mod:14); the CPU oracle is
// oracle/aesgcm_oracle.c, pinned by the GCM specification's test cases.
//
// One wave per GCM block.  The block's GHASH inputs (ciphertext sub-blocks
// then the length block, m of them) are padded at the front with zeros to
// 64*J slots; lane l takes slots l, l+64, ..., so loads and stores of
// consecutive lanes are consecutive 16-byte words.  Each lane runs AES-CTR on
// its sub-blocks and a Horner GHASH with multiplier H^64,
//     acc_l = sum_j Y[l+64j] * (H^64)^(J-1-j),
// then multiplies by H^(64-l); the XOR over lanes is the GHASH
//     sum_t Y[t] * H^(64J - t)
// (leading zero slots do not change it).  Lanes whose first slot is padding
// compute AES(K, J0) instead, which masks the tag.
//
// AES: T-tables in LDS, round keys in SGPRs.  GHASH: the Horner steps on an
// 8-bit table of H^64 (16 lookups per product), the final products by
// H^(64-l) on Shoup's 4-bit tables of H^1..H^64, all in LDS (20 KB per key,
// built on the host by gcm_prepare).  36.6 KB of LDS and 128 VGPRs per
// workgroup of 4 waves: four workgroups per CU.
//
// Three kernels.  gcm_blocks: segments of one block count, a fixed number of
// workgroups each (gcm_launch).  gcm_blocks_sized: segments that each have
// their own block count (ec_gcm_seal_segments_sized / ec_gcm_open_segments_sized);
// a workgroup finds its segment's descriptor through a per-pass map, and the
// segment's workgroups run the same stride loop over its blocks
// (gcm_launch_sized, gcm_sized_geom.hpp).  gcm_open_ranged: the
// sized open over a run of covered blocks per segment, block r under nonce +
// (first block + r), every block authenticated whole and only the wanted bytes
// [head, head + length) stored, at any alignment (ec_gcm_open_ranges_sized,
// range_geom.hpp).
//
// A fourth kernel stands beside them: gcm_messages, the cipher's other form in
// the stream layer -- one whole message of any length per seal, no blocks, a raw
// 32-byte key per message and no GcmSched (ec_gcm_seal_messages /
// ec_gcm_open_messages; gcm_msg_device.hpp, gcm_msg_geom.hpp).  It
// shares the T-table AES below and nothing of the per-key GHASH tables.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "aesgcm.hpp"
#include "gcm_msg_device.hpp"
#include "gcm_msg_geom.hpp"

namespace uplink_ec {
namespace {

// ---- tables (host and device) ----

constexpr uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
constexpr uint8_t gmul8(uint8_t a, uint8_t b) {
    uint8_t r = 0;
    for (int i = 0; i < 8; i++) {
        if (b & 1) r ^= a;
        a = xtime(a);
        b >>= 1;
    }
    return r;
}

struct AesTables {
    uint8_t sbox[256];
    uint32_t t0[256];
    constexpr AesTables() : sbox{}, t0{} {
        uint8_t ex[256] = {}, lg[256] = {};  // powers of the generator 3
        uint8_t p = 1;
        for (int i = 0; i < 255; i++) {
            ex[i] = p;
            lg[p] = (uint8_t)i;
            p = (uint8_t)(p ^ xtime(p));
        }
        for (int x = 0; x < 256; x++) {
            const uint8_t inv = x ? ex[(255 - lg[x]) % 255] : 0;  // multiplicative inverse mod 0x11b
            uint8_t s = inv, r = inv;
            for (int i = 0; i < 4; i++) {  // affine map
                r = (uint8_t)((r << 1) | (r >> 7));
                s ^= r;
            }
            sbox[x] = (uint8_t)(s ^ 0x63);
        }
        for (int x = 0; x < 256; x++) {
            const uint8_t s = sbox[x];
            t0[x] = (uint32_t)xtime(s) << 24 | (uint32_t)s << 16 | (uint32_t)s << 8 | (uint8_t)(xtime(s) ^ s);
        }
    }
};
constexpr AesTables kAes{};
__device__ constexpr AesTables kAesDev{};

constexpr uint32_t ror32(uint32_t x, int n) { return n ? (x >> n) | (x << (32 - n)) : x; }

// Shoup's reduction constants for a 4-bit shift, placed at the top of word 0
__device__ constexpr uint32_t kRem4[16] = {0x0000u << 16, 0x1C20u << 16, 0x3840u << 16, 0x2460u << 16,
                                           0x7080u << 16, 0x6CA0u << 16, 0x48C0u << 16, 0x54E0u << 16,
                                           0xE100u << 16, 0xFD20u << 16, 0xD940u << 16, 0xC560u << 16,
                                           0x9180u << 16, 0x8DA0u << 16, 0xA9C0u << 16, 0xB5E0u << 16};

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00010203u); }

// Reduction constants for an 8-bit shift (the bits of the shifted-out byte
// folded back through x^128 = x^7 + x^2 + x + 1, reflected): the top 16 bits of word 0
struct Rem8 {
    uint16_t r[256];
    constexpr Rem8() : r{} {
        for (int b = 0; b < 256; b++) {
            uint64_t hi = 0, lo = (uint64_t)b;
            for (int i = 0; i < 8; i++) {
                const uint64_t carry = lo & 1;
                lo = (lo >> 1) | (hi << 63);
                hi = (hi >> 1) ^ (carry ? 0xE100000000000000ull : 0);
            }
            r[b] = (uint16_t)(hi >> 48);
        }
    }
};
__device__ constexpr Rem8 kRem8{};

// T-table layout: T0 alone, replicated kCopies times with copy c of entry x
// at word x*kCopies + c; lane l reads copy l % kCopies; T1..T3 are rotations
// of T0.  16 copies (16 KB) with four workgroups per CU beat 32 copies with
// three (DESIGN.md §4c has the measured alternatives).
#ifndef UPLINK_GCM_COPIES  // (-D for A/B builds)
#define UPLINK_GCM_COPIES 16
#endif
constexpr int kCopies = UPLINK_GCM_COPIES;

struct Lds {
    uint32_t t[256 * kCopies];
    uint32_t rem[16];
    uint32_t htab[64][16][4];    // H^1..H^64
    uint32_t h8[256][4];         // byte * H^64
    uint16_t rem8[256];          // (16 bits each: with three workgroups' tables the CU's LDS is full)
};

// Tk[x] for this lane (LdsT: a workgroup's LDS whose member t is the T-table)
template <int k, class LdsT>
__device__ __forceinline__ uint32_t T(const LdsT &L, uint32_t x, uint32_t copy) {
    const uint32_t v = L.t[x * kCopies + copy];
    return k ? __builtin_amdgcn_alignbit(v, v, 8 * k) : v;
}

// AES-256 of the big-endian words s[4] with round keys rk (SGPRs), T-tables in LDS
template <class LdsT>
__device__ __forceinline__ void aes_encrypt(uint32_t (&s)[4], const uint32_t *__restrict__ rk, const LdsT &L) {
    const uint32_t cp = threadIdx.x % kCopies;
    uint32_t a = s[0] ^ rk[0], b = s[1] ^ rk[1], c = s[2] ^ rk[2], d = s[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 14; r++) {
        const uint32_t e = T<0>(L, a >> 24, cp) ^ T<1>(L, (b >> 16) & 255, cp) ^ T<2>(L, (c >> 8) & 255, cp) ^ T<3>(L, d & 255, cp) ^ rk[4 * r];
        const uint32_t f = T<0>(L, b >> 24, cp) ^ T<1>(L, (c >> 16) & 255, cp) ^ T<2>(L, (d >> 8) & 255, cp) ^ T<3>(L, a & 255, cp) ^ rk[4 * r + 1];
        const uint32_t g = T<0>(L, c >> 24, cp) ^ T<1>(L, (d >> 16) & 255, cp) ^ T<2>(L, (a >> 8) & 255, cp) ^ T<3>(L, b & 255, cp) ^ rk[4 * r + 2];
        const uint32_t h = T<0>(L, d >> 24, cp) ^ T<1>(L, (a >> 16) & 255, cp) ^ T<2>(L, (b >> 8) & 255, cp) ^ T<3>(L, c & 255, cp) ^ rk[4 * r + 3];
        a = e, b = f, c = g, d = h;
    }
    // last round: S-box bytes, picked out of the T-tables (T2 MSB, T3 byte 2, T0 byte 1, T1 LSB = S[x])
    s[0] = ((T<2>(L, a >> 24, cp) & 0xff000000u) | (T<3>(L, (b >> 16) & 255, cp) & 0x00ff0000u) |
            (T<0>(L, (c >> 8) & 255, cp) & 0x0000ff00u) | (T<1>(L, d & 255, cp) & 0xffu)) ^ rk[56];
    s[1] = ((T<2>(L, b >> 24, cp) & 0xff000000u) | (T<3>(L, (c >> 16) & 255, cp) & 0x00ff0000u) |
            (T<0>(L, (d >> 8) & 255, cp) & 0x0000ff00u) | (T<1>(L, a & 255, cp) & 0xffu)) ^ rk[57];
    s[2] = ((T<2>(L, c >> 24, cp) & 0xff000000u) | (T<3>(L, (d >> 16) & 255, cp) & 0x00ff0000u) |
            (T<0>(L, (a >> 8) & 255, cp) & 0x0000ff00u) | (T<1>(L, b & 255, cp) & 0xffu)) ^ rk[58];
    s[3] = ((T<2>(L, d >> 24, cp) & 0xff000000u) | (T<3>(L, (a >> 16) & 255, cp) & 0x00ff0000u) |
            (T<0>(L, (b >> 8) & 255, cp) & 0x0000ff00u) | (T<1>(L, c & 255, cp) & 0xffu)) ^ rk[59];
}

// z = x * E in GF(2^128) (GCM bit order), E given by its 4-bit table; words big-endian
__device__ __forceinline__ void gf_mul(uint32_t (&z)[4], const uint32_t (&x)[4], const uint32_t (*tab)[4],
                                       const uint32_t *rem) {
    uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        const uint32_t byte = (x[i >> 2] >> ((3 - (i & 3)) * 8)) & 0xff;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t nib = h ? byte >> 4 : byte & 15;
            if (i != 15 || h) {
                const uint32_t r = rem[z3 & 15];
                z3 = __builtin_amdgcn_alignbit(z2, z3, 4);
                z2 = __builtin_amdgcn_alignbit(z1, z2, 4);
                z1 = __builtin_amdgcn_alignbit(z0, z1, 4);
                z0 = (z0 >> 4) ^ r;
            }
            z0 ^= tab[nib][0], z1 ^= tab[nib][1], z2 ^= tab[nib][2], z3 ^= tab[nib][3];
        }
    }
    z[0] = z0, z[1] = z1, z[2] = z2, z[3] = z3;
}

// z = x * E with E's 8-bit table (one lookup and one reduction per byte: half
// the steps of gf_mul's 4-bit table)
__device__ __forceinline__ void gf_mul8(uint32_t (&z)[4], const uint32_t (&x)[4], const uint32_t (*tab)[4],
                                        const uint16_t *rem8) {
    uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        const uint32_t byte = (x[i >> 2] >> ((3 - (i & 3)) * 8)) & 0xff;
        if (i != 15) {
            const uint32_t r = (uint32_t)rem8[z3 & 0xff] << 16;
            z3 = __builtin_amdgcn_alignbit(z2, z3, 8);
            z2 = __builtin_amdgcn_alignbit(z1, z2, 8);
            z1 = __builtin_amdgcn_alignbit(z0, z1, 8);
            z0 = (z0 >> 8) ^ r;
        }
        const uint4 t = *reinterpret_cast<const uint4 *>(tab[byte]);
        z0 ^= t.x, z1 ^= t.y, z2 ^= t.z, z3 ^= t.w;
    }
    z[0] = z0, z[1] = z1, z[2] = z2, z[3] = z3;
}

// bytes [0, n) of the 16-byte word at p (n < 16), big-endian words, zero padded
__device__ __forceinline__ void load_tail(const uint8_t *p, uint32_t n, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint32_t i = 0; i < n; i++) w[i >> 2] |= (uint32_t)p[i] << (24 - 8 * (i & 3));
}

// What a GCM block's shape fixes for every block of a launch.
// (in_block a multiple of 16: gcm_block has no short last sub-block)
struct GcmShape {
    uint32_t ib;                  // in_block
    uint32_t slots, steps, pad;   // GHASH inputs (sub-blocks + the length block), Horner steps, leading zero slots
    uint64_t clen_bits;
    __device__ __forceinline__ explicit GcmShape(uint32_t in_block)
        : ib(in_block), slots(in_block / 16 + 1), steps((slots + 63) / 64), pad(steps * 64 - slots),
          clen_bits((uint64_t)in_block * 8) {}
};

// AES tables, reduction constants and key ks's GHASH tables into the workgroup's LDS
__device__ __forceinline__ void gcm_fill_lds(Lds &L, const GcmSched *ks) {
    for (int i = threadIdx.x; i < 256 * kCopies; i += blockDim.x) L.t[i] = kAesDev.t0[i / kCopies];
    if (threadIdx.x < 16) L.rem[threadIdx.x] = kRem4[threadIdx.x];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(&ks->htab[0][0][0]);
        uint4 *dst = reinterpret_cast<uint4 *>(&L.htab[0][0][0]);
        for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) dst[i] = src[i];
        const uint4 *s8 = reinterpret_cast<const uint4 *>(&ks->h64_8[0][0]);
        uint4 *d8 = reinterpret_cast<uint4 *>(&L.h8[0][0]);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) {
            d8[i] = s8[i];
            L.rem8[i] = kRem8.r[i];
        }
    }
    __syncthreads();
}

// the segment's nonce as a little-endian 96-bit integer
__device__ __forceinline__ void gcm_load_nonce(const uint8_t *nonce, uint32_t (&nw)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
        nw[i] = (uint32_t)nonce[4 * i] | (uint32_t)nonce[4 * i + 1] << 8 | (uint32_t)nonce[4 * i + 2] << 16 |
                (uint32_t)nonce[4 * i + 3] << 24;
}

// One GCM block on one wave: block b of a segment whose nonce is nw, read at src
// and written at dst, under the key whose round keys are rk and whose tables are
// in L, in_block a multiple of 16.  The counter blocks, the Horner GHASH with H^64,
// the final products, the tag and (open) its comparison, as gcm_blocks below has
// them in its loop; every global access goes through chk.  gcm_blocks keeps its own
// text: calling this body from it changed its register allocation (scratch 8 / 12
// bytes per lane became 24 / 28), so only gcm_blocks_sized calls it.
//
// Io is how a 16-byte slot of the block is read and written: GcmDenseIo for
// gcm_blocks_sized (aligned slots, every one stored), GcmRangedIo for
// gcm_open_ranged (any alignment, the stores cut to the wanted range).
struct GcmDenseIo {
    template <class Chk>
    __device__ __forceinline__ uint4 load(const Chk &chk, const uint8_t *p) const {
        return chk.in(p, 16) ? *reinterpret_cast<const uint4 *>(p) : make_uint4(0, 0, 0, 0);  // (skipped: zeros)
    }
    // o4: the slot's bytes as big-endian words
    template <class Chk>
    __device__ __forceinline__ void store(const Chk &chk, uint8_t *dst, uint32_t sidx, const uint32_t (&o4)[4]) const {
        if (chk.out(dst + 16ull * sidx, 16))
            *reinterpret_cast<uint4 *>(dst + 16ull * sidx) =
                make_uint4(bswap(o4[0]), bswap(o4[1]), bswap(o4[2]), bswap(o4[3]));
    }
};

template <bool kOpen, class Chk, class Io = GcmDenseIo>
__device__ __forceinline__ void gcm_block(const Lds &L, const uint32_t *__restrict__ rk, const uint32_t (&nw)[3],
                                          uint32_t b, const uint8_t *src, uint8_t *dst, const GcmShape &g, int lane,
                                          int32_t *status, const Chk &chk, const Io &io = Io()) {
    const uint32_t ib = g.ib, slots = g.slots, steps = g.steps, pad = g.pad;
    // nonce + b, little-endian with carry across the 12 bytes; then big-endian words for AES
    uint32_t n0 = nw[0], n1 = nw[1], n2 = nw[2];
    {
        const uint64_t lo = (uint64_t)n0 + (uint32_t)b;
        n0 = (uint32_t)lo;
        const uint64_t mid = (uint64_t)n1 + (lo >> 32);
        n1 = (uint32_t)mid;
        n2 += (uint32_t)(mid >> 32);
    }
    const uint32_t j0w0 = bswap(n0), j0w1 = bswap(n1), j0w2 = bswap(n2);
    uint32_t acc[4] = {0, 0, 0, 0}, ekj0[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < steps; j++) {
        const uint32_t t = (uint32_t)lane + 64 * j;
        const bool is_data = t >= pad && t + 1 < pad + slots;
        const bool is_len = t + 1 == pad + slots;
        const uint32_t sidx = t - pad;
        // every lane runs the AES (no divergent second pass): data lanes on their counter block,
        // padding lanes on J0 (the tag mask), the length-block lane on a value it ignores
        uint32_t ks4[4] = {j0w0, j0w1, j0w2, is_data ? 2 + sidx : 1};
        aes_encrypt(ks4, rk, L);
        uint32_t y[4] = {0, 0, 0, 0};
        if (is_data) {
            uint32_t in4[4], o4[4];
            const uint4 w = io.load(chk, src + 16ull * sidx);
            in4[0] = bswap(w.x), in4[1] = bswap(w.y), in4[2] = bswap(w.z), in4[3] = bswap(w.w);
#pragma unroll
            for (int q = 0; q < 4; q++) o4[q] = in4[q] ^ ks4[q];
            io.store(chk, dst, sidx, o4);
#pragma unroll
            for (int q = 0; q < 4; q++) y[q] = kOpen ? in4[q] : o4[q];
        } else if (is_len) {  // len(A) = 0 || len(C) in bits
            y[2] = (uint32_t)(g.clen_bits >> 32);
            y[3] = (uint32_t)g.clen_bits;
        } else if (j == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) ekj0[q] = ks4[q];
        }
        // Horner step with H^64
        if (j) {
            uint32_t m[4];
            gf_mul8(m, acc, L.h8, L.rem8);
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = m[q] ^ y[q];
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = y[q];
        }
    }
    {
        uint32_t m[4];
        gf_mul(m, acc, L.htab[63 - lane], L.rem);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = m[q];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] ^= __shfl_xor(acc[q], off);
    if (pad == 0) {  // no padding lane computed AES(K, J0): lane 0 does it now
        if (lane == 0) {
            uint32_t k4[4] = {j0w0, j0w1, j0w2, 1};
            aes_encrypt(k4, rk, L);
#pragma unroll
            for (int q = 0; q < 4; q++) ekj0[q] = k4[q];
        }
    }
    if (lane == 0) {
        uint32_t tag[4];
#pragma unroll
        for (int q = 0; q < 4; q++) tag[q] = acc[q] ^ ekj0[q];
        if (kOpen) {
            const uint8_t *given = src + ib;
            bool ok = true;
            if (chk.in(given, 16))
                for (int i = 0; i < 16; i++) ok &= given[i] == (uint8_t)(tag[i >> 2] >> (24 - 8 * (i & 3)));
            if (!ok && chk.status(status)) atomicMin(status, (int32_t)b);
        } else if (chk.out(dst + ib, 16)) {
            for (int i = 0; i < 16; i++) dst[ib + i] = (uint8_t)(tag[i >> 2] >> (24 - 8 * (i & 3)));
        }
    }
}

#ifndef UPLINK_GCM_WAVES_PER_EU  // (-D for A/B builds: a register budget of 512 / this per lane)
#define UPLINK_GCM_WAVES_PER_EU 4
#endif
template <bool kOpen>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(UPLINK_GCM_WAVES_PER_EU))) void gcm_blocks(
    GcmBatch a, uint32_t wgs_per_seg) {
    __shared__ Lds L;
    const uint32_t seg = blockIdx.x / wgs_per_seg;
    const uint32_t wg = blockIdx.x % wgs_per_seg;
    const GcmSched *ks = a.sched + seg;
    for (int i = threadIdx.x; i < 256 * kCopies; i += blockDim.x) L.t[i] = kAesDev.t0[i / kCopies];
    if (threadIdx.x < 16) L.rem[threadIdx.x] = kRem4[threadIdx.x];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(&ks->htab[0][0][0]);
        uint4 *dst = reinterpret_cast<uint4 *>(&L.htab[0][0][0]);
        for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) dst[i] = src[i];
        const uint4 *s8 = reinterpret_cast<const uint4 *>(&ks->h64_8[0][0]);
        uint4 *d8 = reinterpret_cast<uint4 *>(&L.h8[0][0]);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) {
            d8[i] = s8[i];
            L.rem8[i] = kRem8.r[i];
        }
    }
    __syncthreads();
    uint32_t rk[60];
#pragma unroll
    for (int i = 0; i < 60; i++) rk[i] = ks->rk[i];  // uniform: scalar loads

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ib = a.in_block;
    const uint32_t nsub = (ib + 15) / 16, tail = ib & 15;
    const uint32_t slots = nsub + 1;  // + the length block
    const uint32_t steps = (slots + 63) / 64, pad = steps * 64 - slots;
    const uint8_t *nonce = a.nonces + 12ull * seg;
    uint32_t nw[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        nw[i] = (uint32_t)nonce[4 * i] | (uint32_t)nonce[4 * i + 1] << 8 | (uint32_t)nonce[4 * i + 2] << 16 |
                (uint32_t)nonce[4 * i + 3] << 24;  // little-endian 96-bit integer
    const uint64_t clen_bits = (uint64_t)ib * 8;

    for (uint32_t b = wg * 4 + wave; b < a.nblocks; b += wgs_per_seg * 4) {
        // nonce + b, little-endian with carry across the 12 bytes; then big-endian words for AES
        uint32_t n0 = nw[0], n1 = nw[1], n2 = nw[2];
        {
            const uint64_t lo = (uint64_t)n0 + (uint32_t)b;
            n0 = (uint32_t)lo;
            const uint64_t mid = (uint64_t)n1 + (lo >> 32);
            n1 = (uint32_t)mid;
            n2 += (uint32_t)(mid >> 32);
        }
        const uint32_t j0w0 = bswap(n0), j0w1 = bswap(n1), j0w2 = bswap(n2);
        const uint8_t *src = a.in + (int64_t)seg * a.in_seg_stride + (int64_t)b * a.in_blk_stride;
        uint8_t *dst = a.out + (int64_t)seg * a.out_seg_stride + (int64_t)b * a.out_blk_stride;
        uint32_t acc[4] = {0, 0, 0, 0}, ekj0[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < steps; j++) {
            const uint32_t t = (uint32_t)lane + 64 * j;
            const bool is_data = t >= pad && t + 1 < pad + slots;
            const bool is_len = t + 1 == pad + slots;
            const uint32_t sidx = t - pad;
            // every lane runs the AES (no divergent second pass): data lanes on their counter block,
            // padding lanes on J0 (the tag mask), the length-block lane on a value it ignores
            uint32_t ks4[4] = {j0w0, j0w1, j0w2, is_data ? 2 + sidx : 1};
            aes_encrypt(ks4, rk, L);
            uint32_t y[4] = {0, 0, 0, 0};
            if (is_data) {
                const uint32_t n = (sidx + 1 == nsub && tail) ? tail : 16;
                uint32_t in4[4];
                if (n == 16) {
                    const uint4 w = *reinterpret_cast<const uint4 *>(src + 16ull * sidx);
                    in4[0] = bswap(w.x), in4[1] = bswap(w.y), in4[2] = bswap(w.z), in4[3] = bswap(w.w);
                } else {
                    load_tail(src + 16ull * sidx, n, in4);
                }
                uint32_t o4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) o4[q] = in4[q] ^ ks4[q];
                if (n == 16) {
                    *reinterpret_cast<uint4 *>(dst + 16ull * sidx) =
                        make_uint4(bswap(o4[0]), bswap(o4[1]), bswap(o4[2]), bswap(o4[3]));
                } else {
                    for (uint32_t i = 0; i < n; i++) dst[16ull * sidx + i] = (uint8_t)(o4[i >> 2] >> (24 - 8 * (i & 3)));
                    // GHASH sees the zero-padded ciphertext
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t lo = 4 * q;
                        const uint32_t keep = n >= lo + 4 ? 0xffffffffu : n <= lo ? 0u : ~(0xffffffffu >> (8 * (n - lo)));
                        o4[q] &= keep;
                        in4[q] &= keep;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) y[q] = kOpen ? in4[q] : o4[q];
            } else if (is_len) {  // len(A) = 0 || len(C) in bits
                y[2] = (uint32_t)(clen_bits >> 32);
                y[3] = (uint32_t)clen_bits;
            } else if (j == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) ekj0[q] = ks4[q];
            }
            // Horner step with H^64
            if (j) {
                uint32_t m[4];
                gf_mul8(m, acc, L.h8, L.rem8);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = m[q] ^ y[q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = y[q];
            }
        }
        {
            uint32_t m[4];
            gf_mul(m, acc, L.htab[63 - lane], L.rem);
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = m[q];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] ^= __shfl_xor(acc[q], off);
        if (pad == 0) {  // no padding lane computed AES(K, J0): lane 0 does it now
            if (lane == 0) {
                uint32_t k4[4] = {j0w0, j0w1, j0w2, 1};
                aes_encrypt(k4, rk, L);
#pragma unroll
                for (int q = 0; q < 4; q++) ekj0[q] = k4[q];
            }
        }
        if (lane == 0) {
            uint32_t tag[4];
#pragma unroll
            for (int q = 0; q < 4; q++) tag[q] = acc[q] ^ ekj0[q];
            if (kOpen) {
                const uint8_t *given = src + ib;
                bool ok = true;
                for (int i = 0; i < 16; i++) ok &= given[i] == (uint8_t)(tag[i >> 2] >> (24 - 8 * (i & 3)));
                if (!ok) atomicMin(a.status + seg, (int32_t)b);
            } else {
                for (int i = 0; i < 16; i++) dst[ib + i] = (uint8_t)(tag[i >> 2] >> (24 - 8 * (i & 3)));
            }
        }
    }
}

// ---- segments of different sizes in one launch (aesgcm.hpp GcmSizedArgs) ----

[[maybe_unused]] constexpr int kSiteGcmIn = 41, kSiteGcmOut = 42, kSiteGcmStatus = 43, kSiteGcmPad = 44;  // (checked build)

// Checked build: a segment's declared extents -- its input, its output and the
// call's status words.  An access outside is skipped and its site recorded (as
// blake3.hip in_piece / list_store_ok); in the product build every access passes
// and the struct is empty.
template <int kSiteIn, int kSiteOut, int kSiteStatus>
struct GcmCheck {
#ifdef UPLINK_EC_CHECKED
    const uint8_t *in_lo, *out_lo;
    uint64_t in_len, out_len;
    const int32_t *st_lo;
    uint32_t nseg;
    uint32_t *flag;
    __device__ __forceinline__ bool span(const void *p, uint32_t bytes, const uint8_t *lo, uint64_t len, int site) const {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        if (q >= lo && (uint64_t)(q - lo) + bytes <= len) return true;
        if (flag) atomicCAS(flag, 0u, (uint32_t)site);
        return false;
    }
    __device__ __forceinline__ bool in(const void *p, uint32_t bytes) const { return span(p, bytes, in_lo, in_len, kSiteIn); }
    __device__ __forceinline__ bool out(const void *p, uint32_t bytes) const { return span(p, bytes, out_lo, out_len, kSiteOut); }
    __device__ __forceinline__ bool status(const void *p) const {
        return span(p, 4, reinterpret_cast<const uint8_t *>(st_lo), 4ull * nseg, kSiteStatus);
    }
#else
    __device__ __forceinline__ bool in(const void *, uint32_t) const { return true; }
    __device__ __forceinline__ bool out(const void *, uint32_t) const { return true; }
    __device__ __forceinline__ bool status(const void *) const { return true; }
#endif
};
using GcmSizedCheck = GcmCheck<kSiteGcmIn, kSiteGcmOut, kSiteGcmStatus>;

// A workgroup finds its segment through the pass's map (uniform per workgroup:
// scalar loads), fills its LDS with that segment's key and runs gcm_blocks' stride
// loop over the segment's blocks on the segment's own workgroups.
template <bool kOpen>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(UPLINK_GCM_WAVES_PER_EU))) void gcm_blocks_sized(
    GcmSizedArgs a) {
    __shared__ Lds L;
    const GcmSizedDesc *d = a.desc + a.map[blockIdx.x];
    const uint32_t seg = d->seg, nblocks = d->nblocks, wgs = d->wgs;
    const uint32_t wg = blockIdx.x - d->wg0;
    const uint8_t *in = d->in;
    uint8_t *out = d->out;
    const GcmSched *ks = a.sched + seg;
    gcm_fill_lds(L, ks);
    uint32_t rk[60];
#pragma unroll
    for (int i = 0; i < 60; i++) rk[i] = ks->rk[i];  // uniform: scalar loads

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GcmShape g(a.in_block);
    uint32_t nw[3];
    gcm_load_nonce(a.nonces + 12ull * seg, nw);
    const uint64_t in_blk = kOpen ? (uint64_t)g.ib + 16 : g.ib, out_blk = kOpen ? g.ib : (uint64_t)g.ib + 16;
    GcmSizedCheck chk;
#ifdef UPLINK_EC_CHECKED
    chk = {in, out, in_blk * nblocks, out_blk * nblocks, a.status, a.nseg, a.chk_flag};
#endif

    for (uint32_t b = wg * 4 + wave; b < nblocks; b += wgs * 4)
        gcm_block<kOpen>(L, rk, nw, b, in + in_blk * b, out + out_blk * b, g, lane, a.status + seg, chk);
}

// One workgroup per segment of the pass: its descriptor from the host's staging to
// device memory, its workgroups' entries of the map, and, for a segment given by its
// data length, PadReader's padding behind the data (the bytes ec_pad_segments
// writes).  rs_encode_sized_prep's counterpart (rs_encode_sized.hip).
__global__ __launch_bounds__(256) void gcm_sized_prep(const GcmSizedStage *stage, GcmSizedDesc *desc, uint32_t *map,
                                                      uint32_t in_block, uint32_t *chk_flag) {
    const GcmSizedStage *st = stage + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(&st->d);
        uint64_t *dst = reinterpret_cast<uint64_t *>(desc + blockIdx.x);
        for (uint32_t i = tid; i < sizeof(GcmSizedDesc) / 8; i += blockDim.x) dst[i] = src[i];
    }
    uint32_t *m = map + st->d.wg0;
    const uint32_t wgs = st->d.wgs;
    for (uint32_t i = tid; i < wgs; i += blockDim.x) m[i] = blockIdx.x;
    // the padding: at most a block and 3 bytes
    const uint32_t p = st->pad;
    if (p) {
        uint8_t *tail = const_cast<uint8_t *>(st->d.in) + st->data_len;
        for (uint32_t i = tid; i < p; i += blockDim.x) {
            uint8_t v = (uint8_t)p;
            if (i + 4 >= p) v = (uint8_t)(p >> (8 * (p - 1 - i)));  // last 4 bytes: big-endian p
#ifdef UPLINK_EC_CHECKED
            if (st->data_len + i >= (uint64_t)st->d.nblocks * in_block) {
                if (chk_flag) atomicCAS(chk_flag, 0u, (uint32_t)kSiteGcmPad);
                continue;
            }
#endif
            tail[i] = v;
        }
    }
    (void)in_block, (void)chk_flag;
}

// ---- ranges of segments opened in one launch (aesgcm.hpp GcmRangedArgs) ----

// Slot I/O of one covered block of a ranged open.  The block's plaintext byte j
// belongs at out[rel + j] (rel = the block's first byte minus head, negative only
// in the first block) and is stored only when that index is inside [0, len).
// kAligned: every source slot and every output slot address of the segment is
// 16-byte aligned (aligned pointers, head a multiple of 16): the uint4 load and
// store of the dense kernel, byte stores only in the slot the range ends in.
// Otherwise no uint4 or uint32_t is dereferenced at an address that is not so
// aligned: a misaligned source slot is read byte by byte, a whole slot whose
// output is 4-byte aligned is stored as four words and everything else as bytes.
template <bool kAligned>
struct GcmRangedIo {
    uint8_t *out;
    int64_t rel;
    uint64_t len;
    bool src16;  // the segment's source slots are 16-byte aligned

    template <class Chk>
    __device__ __forceinline__ uint4 load(const Chk &chk, const uint8_t *p) const {
        if (kAligned || src16) return GcmDenseIo().load(chk, p);
        uint32_t w[4] = {0, 0, 0, 0};
        if (chk.in(p, 16)) {
#pragma unroll
            for (int i = 0; i < 16; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }

    template <class Chk>
    __device__ __forceinline__ void store(const Chk &chk, uint8_t *, uint32_t sidx, const uint32_t (&o4)[4]) const {
        const int64_t at = rel + 16ll * sidx;        // the slot's byte 0 in out
        const int64_t left = (int64_t)len - at;      // bytes from there to the end of the range
        if (at >= 0 && left >= 16) {                 // a whole slot
            uint8_t *q = out + at;
            if (kAligned || (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
                if (chk.out(q, 16))
                    *reinterpret_cast<uint4 *>(q) = make_uint4(bswap(o4[0]), bswap(o4[1]), bswap(o4[2]), bswap(o4[3]));
                return;
            }
            if ((reinterpret_cast<uintptr_t>(q) & 3) == 0) {
                if (chk.out(q, 16)) {
                    uint32_t *w = reinterpret_cast<uint32_t *>(q);
#pragma unroll
                    for (int i = 0; i < 4; i++) w[i] = bswap(o4[i]);
                }
                return;
            }
        }
        if (at <= -16 || left <= 0) return;  // nothing of this slot is wanted
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (at + i >= 0 && i < left && chk.out(out + (at + i), 1))
                out[at + i] = (uint8_t)(o4[i >> 2] >> (24 - 8 * (i & 3)));
    }
};

// The stride loop of gcm_blocks_sized over a segment's covered blocks: relative
// block r is absolute block fb + r for the nonce and the status word.
template <bool kAligned>
__device__ __forceinline__ void gcm_ranged_blocks(const Lds &L, const uint32_t *__restrict__ rk, const uint32_t (&nw)[3],
                                                  const GcmRangedDesc *d, uint32_t wg, const GcmShape &g,
                                                  int32_t *status, const GcmSizedCheck &chk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *in = d->in;
    uint8_t *out = d->out;
    const uint32_t nblocks = d->nblocks, fb = d->first_block, wgs = d->wgs;
    const int64_t head = d->head;
    const uint64_t len = d->length, in_blk = (uint64_t)g.ib + 16;
    const bool src16 = (reinterpret_cast<uintptr_t>(in) & 15) == 0;  // (the block stride is a multiple of 16)
    for (uint32_t r = wg * 4 + wave; r < nblocks; r += wgs * 4) {
        const GcmRangedIo<kAligned> io{out, (int64_t)((uint64_t)r * g.ib) - head, len, src16};
        gcm_block<true>(L, rk, nw, fb + r, in + in_blk * r, out, g, lane, status, chk, io);
    }
}

// gcm_blocks_sized<true> with a first block, a head and a length per segment: the
// workgroup -> segment map, the LDS fill and the block body are the same; the
// segment's flag picks the slot I/O (uniform per workgroup).  kMixed false: a pass
// in which no segment has the flag, compiled without the bytewise path.
template <bool kMixed>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(UPLINK_GCM_WAVES_PER_EU))) void gcm_open_ranged(
    GcmRangedArgs a) {
    __shared__ Lds L;
    const GcmRangedDesc *d = a.desc + a.map[blockIdx.x];
    const uint32_t seg = d->seg;
    const uint32_t wg = blockIdx.x - d->wg0;
    const GcmSched *ks = a.sched + seg;
    gcm_fill_lds(L, ks);
    uint32_t rk[60];
#pragma unroll
    for (int i = 0; i < 60; i++) rk[i] = ks->rk[i];  // uniform: scalar loads

    const GcmShape g(a.in_block);
    uint32_t nw[3];
    gcm_load_nonce(a.nonces + 12ull * seg, nw);
    GcmSizedCheck chk;
#ifdef UPLINK_EC_CHECKED
    chk = {d->in, d->out, ((uint64_t)g.ib + 16) * d->nblocks, d->length, a.status, a.nseg, a.chk_flag};
#endif
    if (kMixed && (d->flags & kGcmRangedBytewise))
        gcm_ranged_blocks<false>(L, rk, nw, d, wg, g, a.status + seg, chk);
    else
        gcm_ranged_blocks<true>(L, rk, nw, d, wg, g, a.status + seg, chk);
}

// One workgroup per segment of the pass: its descriptor from the host's staging to
// device memory and its workgroups' entries of the map (as gcm_sized_prep).
__global__ __launch_bounds__(256) void gcm_ranged_prep(const GcmRangedDesc *stage, GcmRangedDesc *desc, uint32_t *map) {
    const GcmRangedDesc *st = stage + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(st);
    uint64_t *dst = reinterpret_cast<uint64_t *>(desc + blockIdx.x);
    for (uint32_t i = tid; i < sizeof(GcmRangedDesc) / 8; i += blockDim.x) dst[i] = src[i];
    uint32_t *m = map + st->wg0;
    const uint32_t wgs = st->wgs;
    for (uint32_t i = tid; i < wgs; i += blockDim.x) m[i] = blockIdx.x;
}

// ---- one-shot messages, a raw key each (aesgcm.hpp GcmMsgArgs) ----

[[maybe_unused]] constexpr int kSiteMsgIn = 51, kSiteMsgOut = 52, kSiteMsgStatus = 53;  // (checked build)
using GcmMsgCheck = GcmCheck<kSiteMsgIn, kSiteMsgOut, kSiteMsgStatus>;

// The multiply by the wave's current multiplier (gcm_msg_device.hpp): 1, on a
// 4-bit table of it that 16 lanes of the wave build in LDS; 0, bit by bit with the
// multiplier's run of shifts in scalar registers.  DESIGN.md 4n has both measured.
#ifndef UPLINK_GCM_MSG_MUL  // (-D for A/B builds)
#define UPLINK_GCM_MSG_MUL 1
#endif

struct MsgLds {
    uint32_t t[256 * kCopies];
    alignas(16) uint32_t tab[gcmmsg::kWaves][16][4];  // a wave's table of its current multiplier
};

__device__ __forceinline__ gcmmsg::Block msg_uniform(const gcmmsg::Block &b) {  // (the same in every lane: to SGPRs)
    return {{(uint32_t)__builtin_amdgcn_readfirstlane(b.w[0]), (uint32_t)__builtin_amdgcn_readfirstlane(b.w[1]),
             (uint32_t)__builtin_amdgcn_readfirstlane(b.w[2]), (uint32_t)__builtin_amdgcn_readfirstlane(b.w[3])}};
}

struct MsgMulBits {
    gcmmsg::Block m;
    __device__ __forceinline__ void set(const gcmmsg::Block &x, int) { m = msg_uniform(x); }
    __device__ __forceinline__ gcmmsg::Block mul(const gcmmsg::Block &x) const { return gcmmsg::gf_mul_bits(x, m); }
};

// Only the table's own wave touches it, and a wave's LDS accesses are served in
// order: the fences keep the compiler from moving one lane's reads across the
// other lanes' writes.
struct MsgMulTable {
    uint32_t (*tab)[4];
    __device__ __forceinline__ void set(const gcmmsg::Block &x, int lane) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (lane < 16) {
            const gcmmsg::Block e = gcmmsg::gf_table_entry(x, (uint32_t)lane);
            *reinterpret_cast<uint4 *>(tab[lane]) = make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ gcmmsg::Block mul(const gcmmsg::Block &x) const {
        uint32_t (*t)[4] = tab;
        return gcmmsg::gf_mul_table(x, [t](uint32_t n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(t[n]);
            return gcmmsg::Block{{v.x, v.y, v.z, v.w}};
        });
    }
};
#if UPLINK_GCM_MSG_MUL
using MsgMul = MsgMulTable;
#else
using MsgMul = MsgMulBits;
#endif

// How a message's 16-byte slots are read and written.  A slot is read with one
// 16-byte load when the message's source is 16-byte aligned, and written with one
// 16-byte store when its destination is, with four words when that is 4-byte
// aligned; everything else, and the message's short last slot, goes byte by byte.
// No uint4 or uint32_t is dereferenced at an address that is not so aligned.
struct GcmMsgIo {
    bool src16, dst16, dst4;  // (the same for every slot of a message: slots are 16 bytes apart)

    // n bytes at p as a zero-padded block
    __device__ __forceinline__ gcmmsg::Block load(const GcmMsgCheck &chk, const uint8_t *p, uint32_t n) const {
        if (n == 16 && src16) {
            const uint4 w = GcmDenseIo().load(chk, p);
            return {{bswap(w.x), bswap(w.y), bswap(w.z), bswap(w.w)}};
        }
        gcmmsg::Block r = gcmmsg::zero_block();
        if (chk.in(p, n)) {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++)  // (unrolled: no word of r is indexed by a run-time value)
                if (i < n) r.w[i >> 2] |= (uint32_t)p[i] << (24 - 8 * (i & 3));
        }
        return r;
    }
    // the first n bytes of o to q
    __device__ __forceinline__ void store(const GcmMsgCheck &chk, uint8_t *q, uint32_t n, const gcmmsg::Block &o) const {
        if (!chk.out(q, n)) return;
        if (n == 16 && dst16) {
            *reinterpret_cast<uint4 *>(q) = make_uint4(bswap(o.w[0]), bswap(o.w[1]), bswap(o.w[2]), bswap(o.w[3]));
        } else if (n == 16 && dst4) {
            uint32_t *w = reinterpret_cast<uint32_t *>(q);
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = bswap(o.w[i]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++)
                if (i < n) q[i] = gcmmsg::block_byte(o, i);
        }
    }
};

// byte i (0..15) of b without indexing its words by a run-time value
__device__ __forceinline__ uint8_t msg_byte(const gcmmsg::Block &b, uint32_t i) {
    const uint32_t w = i < 8 ? (i < 4 ? b.w[0] : b.w[1]) : (i < 12 ? b.w[2] : b.w[3]);
    return (uint8_t)(w >> (24 - 8 * (i & 3)));
}

// One wave per message, gcmmsg::kWaves messages per workgroup; the seal and the
// open are two instantiations of this body.  The wave expands the message's key
// (the S-box is a byte of the T-table in LDS), takes H = AES_K(0) and AES_K(J0)
// in one AES (even and odd lanes), then every lane takes `rounds` consecutive
// slots of the front-padded message (gcm_msg_geom.hpp): AES-CTR on them (seal)
// and a Horner GHASH with H, while H^rounds is run up beside it; the lanes'
// partial sums are folded pairwise with H^rounds, its square, ... (gcm_msg_device.hpp).
// The open authenticates first and only then runs the counter blocks, so nothing
// of a message whose tag does not verify is released: its output is zeros.
template <bool kOpen>
__global__ __launch_bounds__(64 * gcmmsg::kWaves) void gcm_messages(GcmMsgArgs a) {
    using namespace gcmmsg;
    __shared__ MsgLds L;
    for (int i = threadIdx.x; i < 256 * kCopies; i += blockDim.x) L.t[i] = kAesDev.t0[i / kCopies];
    __syncthreads();  // (the only workgroup barrier: a wave without a message leaves after it)
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q = blockIdx.x * kWaves + wave;
    if (q >= a.n) return;
    const GcmMsgDesc *d = a.desc + q;
    const uint8_t *src = d->in;
    uint8_t *dst = d->out;
    const uint32_t len = d->len, msg = d->msg;
    GcmMsgCheck chk;
#ifdef UPLINK_EC_CHECKED
    chk = {src, dst, (uint64_t)len + (kOpen ? kTagBytes : 0), (uint64_t)len + (kOpen ? 0 : kTagBytes), a.status, a.nmsg,
           a.chk_flag};
#endif
    const GcmMsgIo io{(reinterpret_cast<uintptr_t>(src) & 15) == 0, (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
                      (reinterpret_cast<uintptr_t>(dst) & 3) == 0};

    // the round keys, from the 32 key bytes (any alignment): the same in every lane, then scalar
    uint32_t rk[60];
    {
        const uint8_t *kp = a.keys + 32ull * msg;
        uint32_t kw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kw[i] = __builtin_amdgcn_readfirstlane(load_be32(kp + 4 * i));
        const uint32_t cp = threadIdx.x % kCopies;
        const uint32_t *tt = L.t;
        key_expand(kw, rk, [tt, cp](uint32_t x) { return (tt[x * kCopies + cp] >> 8) & 0xffu; });  // T0 byte 1 = S[x]
#pragma unroll
        for (int i = 0; i < 60; i++) rk[i] = __builtin_amdgcn_readfirstlane(rk[i]);
    }
    uint32_t nw[3];
    {
        const uint8_t *np = a.nonces + 12ull * msg;
#pragma unroll
        for (int i = 0; i < 3; i++) nw[i] = __builtin_amdgcn_readfirstlane(load_be32(np + 4 * i));
    }
    // H = AES_K(0) on the even lanes, AES_K(J0), the tag's mask, on the odd ones
    Block h, ekj0;
    {
        uint32_t s4[4] = {0, 0, 0, 0};
        if (lane & 1) s4[0] = nw[0], s4[1] = nw[1], s4[2] = nw[2], s4[3] = 1;
        aes_encrypt(s4, rk, L);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            h.w[i] = __builtin_amdgcn_readlane(s4[i], 0);
            ekj0.w[i] = __builtin_amdgcn_readlane(s4[i], 1);
        }
    }

    const uint32_t R = rounds(len), pad = front_pad(len), nd = data_slots(len), tail = tail_bytes(len);
    MsgMul mul{};
#if UPLINK_GCM_MSG_MUL
    mul.tab = L.tab[wave];
#endif
    mul.set(h, lane);

    // lane `lane` takes padded slots lane * R .. lane * R + R - 1; the length block is the last of lane 63
    Block acc = zero_block(), hr = h;
    for (uint32_t j = 0; j < R; j++) {
        const uint32_t t = (uint32_t)lane * R + j;
        const bool is_len = t + 1 == R * kLanes;
        const bool is_data = t >= pad && !is_len;
        const uint32_t sidx = t - pad;
        Block y = zero_block();
        if (is_data) {
            const uint32_t n = sidx + 1 == nd ? tail : 16;
            const Block in = io.load(chk, src + 16ull * sidx, n);
            if (kOpen) {
                y = in;
            } else {
                uint32_t ks4[4] = {nw[0], nw[1], nw[2], 2 + sidx};
                aes_encrypt(ks4, rk, L);
                const Block o = in ^ Block{{ks4[0], ks4[1], ks4[2], ks4[3]}};
                io.store(chk, dst + 16ull * sidx, n, o);
                y = keep_bytes(o, n);  // GHASH sees the zero-padded ciphertext
            }
        } else if (is_len) {
            y = length_block(len);
        }
        acc = horner_step(acc, y, mul);
        if (j) hr = mul.mul(hr);  // H^R beside it (the same in every lane)
    }

    // the pairwise combination; a step whose lower lanes hold only front padding is skipped
    const uint32_t steps = combine_steps(len);
    for (uint32_t s = 0; s < steps; s++) {
        const int dist = 1 << s;
        mul.set(hr, lane);
        Block partner;
#pragma unroll
        for (int i = 0; i < 4; i++) partner.w[i] = __shfl_xor(acc.w[i], dist);
        acc = combine_step(acc, partner, (lane & dist) != 0, mul);
        if (s + 1 < steps) hr = mul.mul(hr);
    }
    // lane 63 holds the GHASH (with fewer than six steps the lanes below the folded ones do not)
    Block tag;
#pragma unroll
    for (int i = 0; i < 4; i++) tag.w[i] = __builtin_amdgcn_readlane(acc.w[i], 63) ^ ekj0.w[i];

    if (!kOpen) {
        if (lane < 16 && chk.out(dst + len + lane, 1)) dst[(uint64_t)len + lane] = msg_byte(tag, lane);
        return;
    }
    bool differs = false;
    if (lane < 16 && chk.in(src + len + lane, 1)) differs = src[(uint64_t)len + lane] != msg_byte(tag, lane);
    const bool ok = __ballot(differs) == 0;
    if (lane == 0 && chk.status(a.status + msg)) a.status[msg] = ok ? 0 : 1;
    for (uint32_t j = 0; j < R; j++) {
        const uint32_t t = (uint32_t)lane * R + j;
        if (t < pad || t + 1 == R * kLanes) continue;
        const uint32_t sidx = t - pad;
        const uint32_t n = sidx + 1 == nd ? tail : 16;
        Block o = zero_block();
        if (ok) {
            uint32_t ks4[4] = {nw[0], nw[1], nw[2], 2 + sidx};
            aes_encrypt(ks4, rk, L);
            o = io.load(chk, src + 16ull * sidx, n) ^ Block{{ks4[0], ks4[1], ks4[2], ks4[3]}};
        }
        io.store(chk, dst + 16ull * sidx, n, o);
    }
}

// The pass's descriptors from the host's staging to device memory.
__global__ __launch_bounds__(256) void gcm_msg_prep(const GcmMsgDesc *stage, GcmMsgDesc *desc, uint32_t n) {
    const uint64_t *src = reinterpret_cast<const uint64_t *>(stage);
    uint64_t *dst = reinterpret_cast<uint64_t *>(desc);
    const uint32_t words = n * (uint32_t)(sizeof(GcmMsgDesc) / 8);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// ---- host helpers ----

uint32_t sub_word(uint32_t w) {
    return (uint32_t)kAes.sbox[w >> 24] << 24 | (uint32_t)kAes.sbox[(w >> 16) & 255] << 16 |
           (uint32_t)kAes.sbox[(w >> 8) & 255] << 8 | kAes.sbox[w & 255];
}

void key_expand(const uint8_t key[32], uint32_t rk[60]) {
    for (int i = 0; i < 8; i++)
        rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
    uint8_t rcon = 1;
    for (int i = 8; i < 60; i++) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = sub_word(ror32(t, 24)) ^ ((uint32_t)rcon << 24);
            rcon = xtime(rcon);
        } else if (i % 8 == 4) {
            t = sub_word(t);
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

// 128-bit GCM field element as (hi, lo) big-endian halves
struct U128 {
    uint64_t hi, lo;
};
U128 gf_mul_bits(U128 x, U128 y) {  // GCM spec Algorithm 1
    U128 z{0, 0}, v = y;
    for (int i = 0; i < 128; i++) {
        const uint64_t bit = i < 64 ? (x.hi >> (63 - i)) & 1 : (x.lo >> (127 - i)) & 1;
        if (bit) z.hi ^= v.hi, z.lo ^= v.lo;
        const uint64_t carry = v.lo & 1;
        v.lo = (v.lo >> 1) | (v.hi << 63);
        v.hi = (v.hi >> 1) ^ (carry ? 0xE100000000000000ull : 0);
    }
    return z;
}

// tab[b] = b * e for every byte b (bit 7 of b the coefficient of x^0)
void shoup_table8(U128 e, uint32_t tab[256][4]) {
    U128 t[256] = {};
    t[128] = e;
    U128 v = e;
    for (int i = 64; i > 0; i >>= 1) {
        const uint64_t carry = v.lo & 1;
        v.lo = (v.lo >> 1) | (v.hi << 63);
        v.hi = (v.hi >> 1) ^ (carry ? 0xE100000000000000ull : 0);
        t[i] = v;
    }
    for (int i = 2; i < 256; i <<= 1)
        for (int j = 1; j < i; j++) t[i + j] = U128{t[i].hi ^ t[j].hi, t[i].lo ^ t[j].lo};
    for (int i = 0; i < 256; i++) {
        tab[i][0] = (uint32_t)(t[i].hi >> 32), tab[i][1] = (uint32_t)t[i].hi;
        tab[i][2] = (uint32_t)(t[i].lo >> 32), tab[i][3] = (uint32_t)t[i].lo;
    }
}

void shoup_table(U128 e, uint32_t tab[16][4]) {
    U128 t[16] = {};
    t[8] = e;
    U128 v = e;
    for (int i = 4; i > 0; i >>= 1) {  // t[i] = e * x^(3 - log2 i): one right shift with reduction each
        const uint64_t carry = v.lo & 1;
        v.lo = (v.lo >> 1) | (v.hi << 63);
        v.hi = (v.hi >> 1) ^ (carry ? 0xE100000000000000ull : 0);
        t[i] = v;
    }
    for (int i = 2; i < 16; i <<= 1)
        for (int j = 1; j < i; j++) t[i + j] = U128{t[i].hi ^ t[j].hi, t[i].lo ^ t[j].lo};
    for (int i = 0; i < 16; i++) {
        tab[i][0] = (uint32_t)(t[i].hi >> 32), tab[i][1] = (uint32_t)t[i].hi;
        tab[i][2] = (uint32_t)(t[i].lo >> 32), tab[i][3] = (uint32_t)t[i].lo;
    }
}

}  // namespace

void aes256_encrypt_block(const uint32_t rk[60], const uint8_t in[16], uint8_t out[16]) {
    uint32_t s[4];
    for (int i = 0; i < 4; i++)
        s[i] = ((uint32_t)in[4 * i] << 24 | (uint32_t)in[4 * i + 1] << 16 | (uint32_t)in[4 * i + 2] << 8 | in[4 * i + 3]) ^
               rk[i];
    for (int r = 1; r <= 14; r++) {
        uint8_t b[16];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) b[4 * i + j] = kAes.sbox[(s[(i + j) % 4] >> (24 - 8 * j)) & 255];  // SubBytes+ShiftRows
        for (int i = 0; i < 4; i++) {
            uint8_t *c = b + 4 * i;
            uint8_t m[4] = {c[0], c[1], c[2], c[3]};
            if (r != 14) {  // MixColumns
                m[0] = (uint8_t)(gmul8(c[0], 2) ^ gmul8(c[1], 3) ^ c[2] ^ c[3]);
                m[1] = (uint8_t)(c[0] ^ gmul8(c[1], 2) ^ gmul8(c[2], 3) ^ c[3]);
                m[2] = (uint8_t)(c[0] ^ c[1] ^ gmul8(c[2], 2) ^ gmul8(c[3], 3));
                m[3] = (uint8_t)(gmul8(c[0], 3) ^ c[1] ^ c[2] ^ gmul8(c[3], 2));
            }
            s[i] = ((uint32_t)m[0] << 24 | (uint32_t)m[1] << 16 | (uint32_t)m[2] << 8 | m[3]) ^ rk[4 * r + i];
        }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(s[i] >> (24 - 8 * j));
}

void gcm_prepare(const uint8_t key[32], GcmSched *out) {
    std::memset(out, 0, sizeof *out);
    key_expand(key, out->rk);
    uint8_t zero[16] = {0}, h[16];
    aes256_encrypt_block(out->rk, zero, h);
    U128 H{0, 0};
    for (int i = 0; i < 8; i++) H.hi = H.hi << 8 | h[i], H.lo = H.lo << 8 | h[8 + i];
    U128 p = H;
    for (int k = 0; k < 64; k++) {  // htab[k] = table of H^(k+1)
        shoup_table(p, out->htab[k]);
        if (k == 63) shoup_table8(p, out->h64_8);
        p = gf_mul_bits(p, H);
    }
}

// The grid a launch aims for: 256 CUs times UPLINK_GCM_GRID_PER_CU (1..64, default 32: gcm_launch)
uint32_t gcm_target_grid() {
    static const uint32_t per_cu = [] {
        const char *e = getenv("UPLINK_GCM_GRID_PER_CU");
        const int v = e ? atoi(e) : 32;
        return (uint32_t)(v > 0 && v <= 64 ? v : 32);
    }();
    return 256 * per_cu;
}

hipError_t gcm_launch_sized(const GcmSizedPass &p, bool open, hipStream_t stream) {
    if (p.n == 0 || p.wgs == 0) return hipSuccess;
    if (p.in_block == 0 || p.in_block > (1u << 24) || p.in_block % 16) return hipErrorInvalidValue;
    gcm_sized_prep<<<dim3(p.n), 256, 0, stream>>>(p.stage, p.desc, p.map, p.in_block, p.chk_flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const GcmSizedArgs a{p.desc, p.map, p.sched, p.nonces, p.status, p.chk_flag, p.in_block, p.nseg};
    if (open)
        gcm_blocks_sized<true><<<dim3(p.wgs), 256, 0, stream>>>(a);
    else
        gcm_blocks_sized<false><<<dim3(p.wgs), 256, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t gcm_launch_ranged(const GcmRangedPass &p, hipStream_t stream) {
    if (p.n == 0 || p.wgs == 0) return hipSuccess;
    if (p.in_block == 0 || p.in_block > (1u << 24) || p.in_block % 16) return hipErrorInvalidValue;
    gcm_ranged_prep<<<dim3(p.n), 256, 0, stream>>>(p.stage, p.desc, p.map);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const GcmRangedArgs a{p.desc, p.map, p.sched, p.nonces, p.status, p.chk_flag, p.in_block, p.nseg};
    if (p.mixed)
        gcm_open_ranged<true><<<dim3(p.wgs), 256, 0, stream>>>(a);
    else
        gcm_open_ranged<false><<<dim3(p.wgs), 256, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t gcm_launch_messages(const GcmMsgPass &p, bool open, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > gcmmsg::kPassMessages) return hipErrorInvalidValue;
    const uint32_t words = p.n * (uint32_t)(sizeof(GcmMsgDesc) / 8);
    gcm_msg_prep<<<dim3((words + 255) / 256), 256, 0, stream>>>(p.stage, p.desc, p.n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const GcmMsgArgs a{p.desc, p.keys, p.nonces, p.status, p.chk_flag, p.n, p.nmsg};
    const dim3 grid(gcmmsg::pass_workgroups(p.n)), block(64 * gcmmsg::kWaves);
    if (open)
        gcm_messages<true><<<grid, block, 0, stream>>>(a);
    else
        gcm_messages<false><<<grid, block, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t gcm_launch(const GcmBatch &b, bool open, hipStream_t stream) {
    if (b.nseg == 0 || b.nblocks == 0) return hipSuccess;
    if (b.in_block == 0 || b.in_block > (1u << 24)) return hipErrorInvalidValue;
    // enough workgroups to fill the chip many times over, each looping over blocks of one segment:
    // 32 per CU (8 segments: seal 167.3 us per segment, against 168.3 at 16, 174.7 at 8, 184.0 at
    // 4; profiles/r05/gcm/ab_grid*.json; UPLINK_GCM_GRID_PER_CU for A/B)
    const uint64_t per_cu = gcm_target_grid() / 256;
    uint32_t wgs = (b.nblocks + 3) / 4;
    const uint32_t cap = (uint32_t)((256ull * per_cu + b.nseg - 1) / b.nseg);
    if (wgs > cap) wgs = cap < 1 ? 1 : cap;
    const dim3 grid(b.nseg * wgs);
    if (open)
        gcm_blocks<true><<<grid, 256, 0, stream>>>(b, wgs);
    else
        gcm_blocks<false><<<grid, 256, 0, stream>>>(b, wgs);
    return hipGetLastError();
}

}  // namespace uplink_ec

// ---- C-ABI (include/uplink_ec.h) ----
#include "../../include/uplink_ec.h"

namespace uplink_ec {
namespace {

__global__ void gcm_status_init(int32_t *s, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) s[i] = 0x7fffffff;
}
__global__ void gcm_status_fini(int32_t *s, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && s[i] == 0x7fffffff) s[i] = -1;
}

// PadReader padding written in place after `len` bytes of each segment
__global__ void pad_segments(uint8_t *segs, int64_t stride, uint64_t len, uint32_t p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p) return;
    uint8_t v = (uint8_t)p;
    if (i + 4 >= p) v = (uint8_t)(p >> (8 * (p - 1 - i)));  // last 4 bytes: big-endian p
    segs[(int64_t)blockIdx.y * stride + len + i] = v;
}

int gcm_fail(hipError_t e) { return e == hipSuccess ? EC_OK : (e == hipErrorInvalidValue ? EC_ERR_INVALID_ARG : EC_ERR_DEVICE); }

int gcm_run(const uint8_t *in, size_t nseg, size_t nblocks, size_t in_block, const void *keys, const uint8_t *nonces,
            uint8_t *out, int32_t *status, bool open, hipStream_t st, int64_t in_seg = 0, int64_t out_seg = 0) {
    if (nseg == 0 || nblocks == 0) return EC_OK;
    if (!in || !out || !keys || !nonces || (open && !status)) return EC_ERR_INVALID_ARG;
    if (in_block == 0 || in_block > (1u << 24) || nseg > 0xFFFFFFu || nblocks > 0x7FFFFFFFu) return EC_ERR_UNSUPPORTED;
    const int64_t ob = (int64_t)in_block + 16;
    GcmBatch b{};
    b.in = in;
    b.out = out;
    b.in_blk_stride = open ? ob : (int64_t)in_block;
    b.out_blk_stride = open ? (int64_t)in_block : ob;
    b.in_seg_stride = in_seg ? in_seg : b.in_blk_stride * (int64_t)nblocks;
    b.out_seg_stride = out_seg ? out_seg : b.out_blk_stride * (int64_t)nblocks;
    if (b.in_seg_stride < b.in_blk_stride * (int64_t)nblocks || b.out_seg_stride < b.out_blk_stride * (int64_t)nblocks ||
        ((b.in_seg_stride | b.out_seg_stride) & 15))
        return EC_ERR_INVALID_ARG;
    b.sched = static_cast<const GcmSched *>(keys);
    b.nonces = nonces;
    b.status = status;
    b.nseg = (uint32_t)nseg;
    b.nblocks = (uint32_t)nblocks;
    b.in_block = (uint32_t)in_block;
    const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                         in_block % 16 == 0;
    if (!aligned) return EC_ERR_UNSUPPORTED;  // 16-byte words throughout (storj's 7408-byte blocks qualify)
    const unsigned g = (unsigned)((nseg + 255) / 256);
    if (open) {
        gcm_status_init<<<g, 256, 0, st>>>(status, (uint32_t)nseg);
        if (hipGetLastError() != hipSuccess) return EC_ERR_DEVICE;
    }
    int rc = gcm_fail(gcm_launch(b, open, st));
    if (rc == EC_OK && open) {
        gcm_status_fini<<<g, 256, 0, st>>>(status, (uint32_t)nseg);
        rc = gcm_fail(hipGetLastError());
    }
    return rc;
}

}  // namespace

hipError_t gcm_status_launch(int32_t *status, uint32_t nseg, bool fini, hipStream_t stream) {
    if (nseg == 0) return hipSuccess;
    const unsigned g = (nseg + 255) / 256;
    if (fini)
        gcm_status_fini<<<g, 256, 0, stream>>>(status, nseg);
    else
        gcm_status_init<<<g, 256, 0, stream>>>(status, nseg);
    return hipGetLastError();
}

}  // namespace uplink_ec

using namespace uplink_ec;

extern "C" {

size_t ec_gcm_key_bytes(void) { return sizeof(GcmSched); }

int ec_gcm_prepare_keys(const uint8_t *keys, size_t nkeys, void *dev_keys, ec_stream stream) {
    if (nkeys == 0) return EC_OK;
    if (!keys || !dev_keys) return EC_ERR_INVALID_ARG;
    // pageable staging (a pinned allocation per call costs more than the 16 KB copy)
    std::vector<GcmSched> host(nkeys);
    for (size_t i = 0; i < nkeys; i++) gcm_prepare(keys + 32 * i, &host[i]);
    hipStream_t st = (hipStream_t)stream;
    int rc = hipMemcpyAsync(dev_keys, host.data(), nkeys * sizeof(GcmSched), hipMemcpyHostToDevice, st) == hipSuccess
                 ? EC_OK
                 : EC_ERR_DEVICE;
    if (hipStreamSynchronize(st) != hipSuccess) rc = EC_ERR_DEVICE;  // before the staging buffer goes
    return rc;
}

int ec_gcm_seal_segments(const uint8_t *plain, size_t nseg, size_t nblocks, size_t in_block, const void *dev_keys,
                         const uint8_t *dev_nonces, uint8_t *out, ec_stream stream) {
    return gcm_run(plain, nseg, nblocks, in_block, dev_keys, dev_nonces, out, nullptr, false, (hipStream_t)stream);
}

int ec_gcm_seal_segments_strided(const uint8_t *plain, long long plain_seg_stride, size_t nseg, size_t nblocks,
                                 size_t in_block, const void *dev_keys, const uint8_t *dev_nonces, uint8_t *out,
                                 long long out_seg_stride, ec_stream stream) {
    return gcm_run(plain, nseg, nblocks, in_block, dev_keys, dev_nonces, out, nullptr, false, (hipStream_t)stream,
                   plain_seg_stride, out_seg_stride);
}

int ec_gcm_open_segments_strided(const uint8_t *cipher, long long cipher_seg_stride, size_t nseg, size_t nblocks,
                                 size_t in_block, const void *dev_keys, const uint8_t *dev_nonces, uint8_t *out,
                                 long long out_seg_stride, int32_t *dev_status, ec_stream stream) {
    return gcm_run(cipher, nseg, nblocks, in_block, dev_keys, dev_nonces, out, dev_status, true, (hipStream_t)stream,
                   cipher_seg_stride, out_seg_stride);
}

int ec_gcm_open_segments(const uint8_t *cipher, size_t nseg, size_t nblocks, size_t in_block, const void *dev_keys,
                         const uint8_t *dev_nonces, uint8_t *out, int32_t *dev_status, ec_stream stream) {
    return gcm_run(cipher, nseg, nblocks, in_block, dev_keys, dev_nonces, out, dev_status, true, (hipStream_t)stream);
}

static int gcm_host(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *in, size_t nblocks,
                    size_t in_block, uint8_t *out, long long *bad_block, bool open) {
    if (!key || !nonce || (nblocks && (!in || !out))) return EC_ERR_INVALID_ARG;
    if (bad_block) *bad_block = -1;
    if (nblocks == 0) return EC_OK;
    const size_t ob = in_block + 16;
    const size_t in_bytes = nblocks * (open ? ob : in_block), out_bytes = nblocks * (open ? in_block : ob);
    hipStream_t st = nullptr;
    uint8_t *d = nullptr;
    int rc = EC_OK;
    const size_t a_in = (in_bytes + 255) & ~(size_t)255, a_out = (out_bytes + 255) & ~(size_t)255;
    do {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { rc = EC_ERR_DEVICE; st = nullptr; break; }
        if (hipMalloc(&d, a_in + a_out + sizeof(GcmSched) + 256) != hipSuccess) { rc = EC_ERR_DEVICE; d = nullptr; break; }
        uint8_t *d_in = d, *d_out = d + a_in, *d_key = d_out + a_out, *d_misc = d_key + sizeof(GcmSched);
        rc = ec_gcm_prepare_keys(key, 1, d_key, st);
        if (rc) break;
        if (hipMemcpyAsync(d_misc, nonce, 12, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { rc = EC_ERR_DEVICE; break; }
        int32_t *d_status = reinterpret_cast<int32_t *>(d_misc + 16);
        rc = gcm_run(d_in, 1, nblocks, in_block, d_key, d_misc, d_out, d_status, open, st);
        if (rc) break;
        int32_t status = -1;
        if (hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
            (open && hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            hipStreamSynchronize(st) != hipSuccess) { rc = EC_ERR_DEVICE; break; }
        if (open && status >= 0) {
            if (bad_block) *bad_block = status;
            rc = EC_ERR_AUTH;
        }
    } while (0);
    if (st) (void)hipStreamSynchronize(st);
    if (d) (void)hipFree(d);
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

int ec_pad_segments(uint8_t *segs, size_t nseg, long long seg_stride, size_t data_len, size_t block, ec_stream stream) {
    if (nseg == 0) return EC_OK;
    if (!segs || block == 0 || nseg > 65535) return EC_ERR_INVALID_ARG;
    const uint64_t p = 4 + (block - (data_len + 4) % block) % block;
    if ((long long)(data_len + p) > seg_stride && nseg > 1) return EC_ERR_INVALID_ARG;
    pad_segments<<<dim3((unsigned)((p + 255) / 256), (unsigned)nseg), 256, 0, (hipStream_t)stream>>>(
        segs, seg_stride, data_len, (uint32_t)p);
    return gcm_fail(hipGetLastError());
}

int ec_gcm_seal_host(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *plain, size_t nblocks,
                     size_t in_block, uint8_t *out) {
    return gcm_host(key, nonce, plain, nblocks, in_block, out, nullptr, false);
}

int ec_gcm_open_host(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *cipher, size_t nblocks,
                     size_t in_block, uint8_t *out, long long *bad_block) {
    return gcm_host(key, nonce, cipher, nblocks, in_block, out, bad_block, true);
}

}  // extern "C"
