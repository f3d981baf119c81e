// SHA-256 of erasure pieces, on the GPU: the legacy piece hash algorithm
// (pb.PieceHashAlgorithm_SHA256, private/piecestore/hash.go:15-26; fed by the
// upload's TeeReader, piecestore/upload.go:133,155,270).  FIPS 180-4.
//
// SHA-256 is one serial chain per piece, so the work is laid out one lane per
// piece: sha256_lanes<Geom> runs 64-thread workgroups (one wave each, so that
// the waves of a short list spread over the CUs), every lane walks its own
// piece block by block, and a lane whose piece is done is masked while the
// rest of its wave goes on.  Throughput comes from the number of pieces in the
// call alone.
//
// A launch advances every piece by at most `nblk` blocks; the eight state words
// of a piece that is not done yet are kept in device memory for the next launch
// (stream order), and the launch that reaches a piece's last block writes its 32
// digest bytes.  A lane that finished in an earlier launch returns at once.
//
// Loads: a fast piece (16-byte aligned base and run stride, contiguous or runs of
// a power of two >= 64 bytes) reads a block as four 16-byte words, the next
// block's in flight while this one is compressed; plain loads, not non-temporal
// ones (blake3.hip load_words: the same lane-per-stream pattern).  Any other
// piece assembles the same words from byte loads.  The last one or two blocks
// are built in registers (sha256_device.hpp pad_block); no load touches a byte
// past the piece's length.
#include <hip/hip_runtime.h>

#include "sha256.hpp"
#include "sha256_device.hpp"
#include "sha_list_geom.hpp"

namespace uplink_ec {
namespace {

using namespace sha256;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One lane's piece, as either geometry hands it to the body.
struct Lane {
    const uint8_t *base;
    uint64_t len, run;
    int64_t run_stride;
    int32_t run_shift;
    bool fast;
    uint8_t *hash;
    uint32_t *state;  // its eight carried words (nullptr: one launch finishes every piece)
};

// Checked build: the declared ranges of the digest and of the state stores, and the violation word.
struct Chk {
    uint8_t *hash_lo, *hash_hi;
    uint8_t *state_lo, *state_hi;
    uint32_t *flag;
};
constexpr int kSiteBlock = 41, kSiteWord = 42, kSiteByte = 43, kSiteStateLoad = 44, kSiteStateStore = 45,
              kSiteDigest = 46;  // (checked build)

// Checked build: `bytes` at p lie in the piece's own extent -- [base, base + len)
// of a contiguous piece, run r of a strided one at [base + r*run_stride, + run)
// -- else the access is skipped and its site recorded.  In the product build this
// is `true` and compiles away.
__device__ __forceinline__ bool in_piece(const Lane &l, const Chk &c, const uint8_t *p, uint32_t bytes, int site) {
#ifdef UPLINK_EC_CHECKED
    if (!c.flag) return true;
    const int64_t off = p - l.base;
    bool ok = off >= 0;
    if (ok && l.run_stride <= 0) ok = (uint64_t)off + bytes <= l.len;
    if (ok && l.run_stride > 0) {
        const uint64_t r = (uint64_t)off / (uint64_t)l.run_stride, w = (uint64_t)off % (uint64_t)l.run_stride;
        ok = w + bytes <= l.run && r * l.run + w + bytes <= l.len;
    }
    if (!ok) atomicCAS(c.flag, 0u, (uint32_t)site);
    return ok;
#else
    (void)l, (void)c, (void)p, (void)bytes, (void)site;
    return true;
#endif
}

// Checked build: 32 bytes at p lie in the digest range, or in the state range.
__device__ __forceinline__ bool range_ok(const Chk &c, const void *p, bool state, int site) {
#ifdef UPLINK_EC_CHECKED
    if (!c.flag) return true;
    const uint8_t *q = static_cast<const uint8_t *>(p);
    const uint8_t *lo = state ? c.state_lo : c.hash_lo, *hi = state ? c.state_hi : c.hash_hi;
    if (q < lo || q + 32 > hi) {
        atomicCAS(c.flag, 0u, (uint32_t)site);
        return false;
    }
#else
    (void)c, (void)p, (void)state, (void)site;
#endif
    return true;
}

// Where a bytewise lane reads next: p, with `left` bytes to the end of p's run.
struct Cursor {
    const uint8_t *p;
    uint64_t left;
    __device__ __forceinline__ void seek(const Lane &l, uint64_t t) {
        const uint64_t q = t / l.run, r = t % l.run;
        p = l.base + (int64_t)q * l.run_stride + r;
        left = l.run - r;
    }
    __device__ __forceinline__ uint32_t next(const Lane &l, const Chk &c) {
        const uint32_t v = in_piece(l, c, p, 1, kSiteByte) ? *p : 0;
        p++;
        if (--left == 0) {
            p += l.run_stride - (int64_t)l.run;
            left = l.run;
        }
        return v;
    }
};

// byte t of a fast piece (t a multiple of 64: the block lies in one run, 16-byte aligned)
__device__ __forceinline__ const uint8_t *fast_at(const Lane &l, uint64_t t) {
    return l.base + (int64_t)(t >> l.run_shift) * l.run_stride + (t & (l.run - 1));
}

// The sixteen words of full block b as they lie in memory (least significant byte first).
__device__ __forceinline__ void load_full(const Lane &l, const Chk &c, Cursor &cur, uint64_t b, uint32_t (&m)[16]) {
    if (l.fast) {
        const uint8_t *p = fast_at(l, 64 * b);
        if (!in_piece(l, c, p, 64, kSiteBlock)) {
#pragma unroll
            for (int i = 0; i < 16; i++) m[i] = 0;
            return;
        }
        const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32x4 v = q[i];
            m[4 * i] = v[0], m[4 * i + 1] = v[1], m[4 * i + 2] = v[2], m[4 * i + 3] = v[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint32_t v = cur.next(l, c);
            v |= cur.next(l, c) << 8;
            v |= cur.next(l, c) << 16;
            v |= cur.next(l, c) << 24;
            m[i] = v;
        }
    }
}

// The message bytes of block b, the piece's last data block or past it (fewer
// than 64 bytes, maybe none), as words with the most significant byte first and
// zeros elsewhere: whole dwords where they lie inside the piece, bytes for the rest.
__device__ __forceinline__ void load_tail(const Lane &l, const Chk &c, Cursor &cur, uint64_t b, uint32_t (&w)[16]) {
    const uint64_t t = 64 * b;
    const uint32_t valid = t < l.len ? (uint32_t)(l.len - t) : 0;  // < 64
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    if (valid == 0) return;
    if (l.fast) {
        const uint8_t *p = fast_at(l, t);
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (4u * i + 4 <= valid && in_piece(l, c, p + 4 * i, 4, kSiteWord))
                w[i] = bswap(*reinterpret_cast<const uint32_t *>(p + 4 * i));
        const uint32_t k = valid >> 2, rem = valid & 3;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 3; j++)
            if (j < rem && in_piece(l, c, p + 4 * k + j, 1, kSiteByte)) v |= (uint32_t)p[4 * k + j] << (24 - 8 * j);
#pragma unroll
        for (int i = 0; i < 16; i++)
            if ((uint32_t)i == k) w[i] = v;  // (k < 16; v == 0 when no byte is left over)
    } else {
#pragma unroll
        for (int i = 0; i < 64; i++)
            if ((uint32_t)i < valid) w[i / 4] |= cur.next(l, c) << (24 - 8 * (i % 4));
    }
}

__device__ __forceinline__ void store_digest(uint8_t *out, const uint32_t (&h)[8]) {
    if (((uintptr_t)out & 3) == 0) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = bswap(h[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h[i / 4] >> (24 - 8 * (i % 4)));
    }
}

// Blocks [blk0, blk0 + nblk) of the lane's piece, as far as it has them.
__device__ __forceinline__ void run_lane(const Lane &l, uint64_t blk0, uint64_t nblk, const Chk &c) {
    const uint64_t nb = blocks_of(l.len);
    if (blk0 >= nb) return;  // finished by an earlier launch
    const uint64_t end = nb - blk0 > nblk ? blk0 + nblk : nb;
    const uint64_t nfull = l.len / 64;
    const uint64_t full_end = end < nfull ? end : nfull;  // this launch's blocks below it are whole data blocks
    uint32_t h[8];
    if (blk0 == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = kInit[i];
    } else {
        uint4 x = make_uint4(0, 0, 0, 0), y = x;
        if (range_ok(c, l.state, true, kSiteStateLoad)) {
            const uint4 *s = reinterpret_cast<const uint4 *>(l.state);
            x = s[0], y = s[1];
        }
        h[0] = x.x, h[1] = x.y, h[2] = x.z, h[3] = x.w, h[4] = y.x, h[5] = y.y, h[6] = y.z, h[7] = y.w;
    }
    Cursor cur{l.base, 0};
    if (!l.fast) cur.seek(l, 64 * blk0);
    uint32_t w[16], nx[16];
    if (blk0 < full_end) load_full(l, c, cur, blk0, w);
    for (uint64_t b = blk0; b < end; b++) {
        const bool more = b + 1 < full_end;
        if (b < full_end) {
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = bswap(w[i]);
        } else {
            load_tail(l, c, cur, b, w);
            pad_block(w, l.len, b);
        }
        if (more) load_full(l, c, cur, b + 1, nx);  // in flight while this block is compressed
        compress(h, w);
        if (more) {
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = nx[i];
        }
    }
    if (end == nb) {
        if (range_ok(c, l.hash, false, kSiteDigest)) store_digest(l.hash, h);
    } else if (range_ok(c, l.state, true, kSiteStateStore)) {
        uint4 *s = reinterpret_cast<uint4 *>(l.state);
        s[0] = make_uint4(h[0], h[1], h[2], h[3]);
        s[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
}

// The list geometry: lane j reads its staged descriptor.
struct ListGeom {
    const ShaDesc *desc;
    uint32_t *state;
    uint32_t lanes;
    __device__ __forceinline__ bool lane(uint32_t j, Lane &l) const {
        if (j >= lanes) return false;
        const ShaDesc d = desc[j];
        if (!d.hash) return false;  // a padding lane
        l = Lane{d.base, d.len, d.run, d.run_stride, d.run_shift, d.fast != 0, d.hash, state + 8ull * j};
        return true;
    }
};

// The uniform geometry: lane j's piece from the launch arguments.
struct UniformGeom {
    const uint8_t *base;
    int64_t piece_stride;
    uint64_t len, run;
    int64_t run_stride;
    int32_t run_shift;
    bool fast;
    uint64_t npieces;
    uint8_t *hashes;
    uint32_t *state;
    __device__ __forceinline__ bool lane(uint32_t j, Lane &l) const {
        if (j >= npieces) return false;
        l = Lane{base + (int64_t)j * piece_stride, len, run, run_stride, run_shift, fast, hashes + 32ull * j,
                 state ? state + 8ull * j : nullptr};
        return true;
    }
};

template <class Geom>
__global__ __launch_bounds__(shalist::kWave) void sha256_lanes(Geom g, uint64_t blk0, uint64_t nblk, Chk c) {
    Lane l;
    if (!g.lane(blockIdx.x * shalist::kWave + threadIdx.x, l)) return;
    run_lane(l, blk0, nblk, c);
}

// The pass's descriptors from the host's pinned memory to device memory, 16 bytes per lane.
__global__ __launch_bounds__(256) void sha256_list_stage(const uint4 *src, uint4 *dst, uint32_t n16) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

}  // namespace

hipError_t sha256_launch_list(const ShaListPass &p, hipStream_t stream) {
    if (p.lanes == 0 || p.launches == 0) return hipSuccess;
    if (!p.h_stage || !p.d_stage || !p.desc || !p.state || (p.stage_bytes & 15) || (p.lanes % shalist::kWave) ||
        p.launch_blocks == 0)
        return hipErrorInvalidValue;
    const uint32_t n16 = (uint32_t)(p.stage_bytes / 16);
    const uint32_t copy_wgs = (n16 + 255) / 256 < 64 ? (n16 + 255) / 256 : 64;
    sha256_list_stage<<<dim3(copy_wgs), 256, 0, stream>>>(static_cast<const uint4 *>(p.h_stage),
                                                           static_cast<uint4 *>(p.d_stage), n16);
    hipError_t e = hipGetLastError();
    const ListGeom g{p.desc, p.state, p.lanes};
    uint8_t *st = reinterpret_cast<uint8_t *>(p.state);
    const Chk c{p.hash_lo, p.hash_hi, st, st + 32ull * p.lanes, p.chk_flag};
    for (uint64_t i = 0; e == hipSuccess && i < p.launches; i++) {
        sha256_lanes<ListGeom><<<dim3(p.lanes / shalist::kWave), shalist::kWave, 0, stream>>>(g, i * p.launch_blocks,
                                                                                            p.launch_blocks, c);
        e = hipGetLastError();
    }
    return e;
}

uint64_t sha256_uniform_launches(const ShaView &v, uint64_t launch_blocks) {
    return v.npieces ? shalist::launches_of(shalist::blocks_of(v.piece_len), launch_blocks) : 0;
}

hipError_t sha256_launch_uniform(const ShaView &v, uint8_t *hashes, uint32_t *state, uint64_t launch_blocks,
                                 hipStream_t stream) {
    if (v.npieces == 0) return hipSuccess;
    if (!hashes || (!v.base && v.piece_len) || launch_blocks == 0 || v.piece_len > shalist::kMaxLen)
        return hipErrorInvalidValue;
    const uint64_t wgs = (v.npieces + shalist::kWave - 1) / shalist::kWave;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t launches = sha256_uniform_launches(v, launch_blocks);
    if (launches > 1 && !state) return hipErrorInvalidValue;
    const b3list::Run r = b3list::run_of({(uint64_t)(uintptr_t)v.base, v.piece_len, v.run, v.run_stride});
    const bool fast = r.run_shift >= 6 && ((uintptr_t)v.base & 15) == 0 && (v.piece_stride & 15) == 0 &&
                      (r.run_stride & 15) == 0;
    const UniformGeom g{v.base, v.piece_stride, v.piece_len, r.run, r.run_stride, r.run_shift, fast,
                        v.npieces, hashes, launches > 1 ? state : nullptr};
    const Chk c{};  // (no context, no violation word: the uniform launches are unchecked, as BLAKE3's)
    hipError_t e = hipSuccess;
    for (uint64_t i = 0; e == hipSuccess && i < launches; i++) {
        sha256_lanes<UniformGeom><<<dim3((uint32_t)wgs), shalist::kWave, 0, stream>>>(g, i * launch_blocks,
                                                                                      launch_blocks, c);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace uplink_ec
