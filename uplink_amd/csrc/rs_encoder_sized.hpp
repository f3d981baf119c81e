// The compile-time-G encoder (rs_encoder.hpp encode_body) restated with a
// geometry per segment (rs_encode_sized.hpp): the same loaders, LDS-DMA, 2-slot
// ring, slicing in place, deferred copy-through, counted vmcnt waits, tile
// queue and wave counts; compute_chunk is the encoder's own.  Restated, not
// shared through a template parameter, as rs_sized.hip restates rs_sets.hip:
// rs_encoder.hpp, its library instantiations and the text hiprtc compiles stay
// byte for byte what they were.  (The diagnostic forms, the A/B variants of the
// store order and the non-deferred copy-through are not restated.)
//
// What is replaced is where a block's columns are: the block's segment comes
// from the pass's map with one uniform load, its descriptor through the
// constant address space (scalar loads, rs_sized.hip); a lane is valid when its
// chunk lies in its segment; input j of chunk (stripe s, t) is at
// in + s k ess + j ess + 16 t, output row r at out + r piece_len + s ess + 16 t
// with the block's own piece_len.  A lane past its segment's end reads its
// segment's column 0, stores nothing for parity and rewrites column 0 with
// itself on the copy-through, so every lane still issues every store and the
// loaders' vmcnt counts stay exact.
#pragma once
#include "rs_encode_sized.hpp"
#include "rs_encoder.hpp"

namespace uplink_ec {
namespace enc {

static_assert(UPLINK_ENC_DEFER_COPY != 0 && UPLINK_ENC_DEFER_ROWS == 0 && UPLINK_ENC_LATE_STORES == 0,
              "the sized encoder restates the product form of encode_body only");

typedef const __attribute__((address_space(4))) EncSizedDesc ConstEncDesc;
typedef const __attribute__((address_space(4))) uint32_t ConstEncMap;

// One block of a tile as a lane sees it: its chunk's first input byte and first
// output byte (of share 0 / row 0), and what a row index is multiplied by.
struct BlockGeo {
    bool v;
    const uint8_t *in;
    uint8_t *out;
    int64_t piece_len;
#ifdef UPLINK_EC_CHECKED
    const uint8_t *in_lo;  // the segment's own input and output extents
    uint8_t *out_lo;
    int64_t in_len, out_len;
#endif
};

// b is wave-uniform.  A block past the pass's last (the second block of the
// last tile of an odd count) is block 0 with no valid lane.
template <int K, int ROWS>
__device__ __forceinline__ BlockGeo block_geo(const EncSizedArgs &a, int64_t b, int lane) {
    const bool have = b < a.total_blocks;
    const int64_t bb = have ? b : 0;
    const uint32_t q = ((ConstEncMap *)a.map)[bb];
    ConstEncDesc *d = (ConstEncDesc *)(a.desc + q);
    const int64_t chunks = d->chunks;
    const int64_t c = (bb - d->block0) * 64 + lane;
    BlockGeo g;
    g.v = have && c < chunks;
    // (chunks fits 32 bits, so a valid lane's index does; an invalid lane's quotient is not used)
    const uint32_t cps = (uint32_t)a.cps;
    const uint32_t s = (uint32_t)c / cps, t = (uint32_t)c - s * cps;
    g.in = d->in + (g.v ? (int64_t)s * K * a.ess + (int64_t)t * 16 : 0);
    g.out = d->out + (g.v ? (int64_t)s * a.ess + (int64_t)t * 16 : 0);
    g.piece_len = d->piece_len;
#ifdef UPLINK_EC_CHECKED
    g.in_lo = d->in;
    g.out_lo = d->out;
    g.in_len = chunks * 16 * K;
    g.out_len = g.piece_len * ROWS;
#endif
    return g;
}

// checked build: an access outside [lo, lo + len) -- the segment's own input or
// its own pieces -- is skipped and its site recorded (as rs_sized.hip in_span)
__device__ __forceinline__ bool enc_in_span(const EncSizedArgs &a, const uint8_t *p, const uint8_t *lo, int64_t len,
                                            int site) {
#ifdef UPLINK_EC_CHECKED
    if (p >= lo && p + 16 <= lo + len) return true;
    if (a.chk_flag) atomicCAS(a.chk_flag, 0u, (uint32_t)site);
    return false;
#else
    (void)a, (void)p, (void)lo, (void)len, (void)site;
    return true;
#endif
}
#ifdef UPLINK_EC_CHECKED
#define UPLINK_ENC_IN_OK(a, p, g, site) enc_in_span(a, p, (g).in_lo, (g).in_len, site)
#define UPLINK_ENC_OUT_OK(a, p, g, site) enc_in_span(a, p, (g).out_lo, (g).out_len, site)
#define UPLINK_ENC_IN_LO(g) (g).in_lo
#else
#define UPLINK_ENC_IN_OK(a, p, g, site) true
#define UPLINK_ENC_OUT_OK(a, p, g, site) true
#define UPLINK_ENC_IN_LO(g) (g).in
#endif

// COPY: the full encode (the systematic data pieces written too); false: the
// parity-only form (EC_FLAG_PARITY_ONLY).
template <int K, int N, int NC, int NL, bool COPY>
__device__ __forceinline__ void encode_sized_body(const EncSizedArgs &a) {
    constexpr int R = N - K;
    constexpr int ROWS = COPY ? N : R;  // rows of a segment's output
    constexpr int ROW0 = COPY ? K : 0;  // row of parity row 0
    constexpr int OPW = (R + NC - 1) / NC;
    constexpr int NCH = chunks_of(K), KC = chunk_size(K);
    constexpr int PER = (KC + NL - 1) / NL;
    constexpr int A = kAhead;
    static_assert(4 * (A - 1) * PER <= 63 && 2 * (2 * A - 1) * PER <= 63 && A == 1,
                  "a loader's VMEM ops in flight must fit the vmcnt counter; deferred stores are counted for 2 slots");
    constexpr int SLOT = KC * 2048;  // bytes
    static_assert(kSlots * SLOT <= 150 * 1024, "LDS ring too large");
    constexpr int K0 = (A + 1 + NCH - 1) / NCH;  // tiles taken before the loop (encode_body)
    __shared__ __attribute__((aligned(16))) u32x4 ring[kSlots * SLOT / 16];
    __shared__ int32_t s_q[8];  // tile of the m-th take, at m & 7
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool loader = wave >= NC;
    const int lw = wave - NC;
    const bool taker = wave == 0 && lane == 0;
    const int64_t P = (a.total_blocks + 1) >> 1;
    const uint32_t ring_addr = (uint32_t)(uint64_t)ring;

    auto take = [&](int m) -> int32_t {
        if (a.queue) return (int32_t)atomicAdd(a.queue, 1u);
        return (int32_t)(blockIdx.x + (int64_t)m * gridDim.x);
    };
    auto ops_of = [&](int ch) -> int {
        const int jn = K - ch * KC < KC ? K - ch * KC : KC;
        return lw < jn ? 2 * ((jn - lw + NL - 1) / NL) : 0;
    };
#ifdef UPLINK_EC_CHECKED
    constexpr bool kCountStores = false;  // the checked build may skip a store: count none (waits longer, never shorter)
#else
    constexpr bool kCountStores = true;
#endif
    // loader: LDS-DMA of this wave's inputs of item (t, ch) into slot sl
    auto issue = [&](int sl, int64_t t, int ch) {
        const BlockGeo gA = block_geo<K, ROWS>(a, t, lane), gB = block_geo<K, ROWS>(a, t + P, lane);
        const int j0 = ch * KC, jn = K - j0 < KC ? K - j0 : KC;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int j = lw + NL * i;
            if (j < jn) {
                const int64_t jo = (int64_t)(j0 + j) * a.ess;
                const uint8_t *pa = gA.in + jo, *pb = gB.in + jo;
                if (!UPLINK_ENC_IN_OK(a, pa, gA, 21)) pa = UPLINK_ENC_IN_LO(gA);
                if (!UPLINK_ENC_IN_OK(a, pb, gB, 21)) pb = UPLINK_ENC_IN_LO(gB);
                const uint32_t d = __builtin_amdgcn_readfirstlane(ring_addr + (uint32_t)(sl * SLOT + j * 2048));
                dma_1k(pa, d);
                dma_1k(pb, d + 1024);
            }
        }
    };
    // loader: the copy-through stores of item (t, ch) -- two per input on every
    // lane, so the wave's count of VMEM ops is exact
    auto copy_out = [&](int64_t t, int ch, const u32x4 *rA, const u32x4 *rB) {
        const BlockGeo gA = block_geo<K, ROWS>(a, t, lane), gB = block_geo<K, ROWS>(a, t + P, lane);
        const int j0 = ch * KC, jn = K - j0 < KC ? K - j0 : KC;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int j = lw + NL * i;
            if (j < jn) {
                uint8_t *qa = gA.out + (int64_t)(j0 + j) * gA.piece_len, *qb = gB.out + (int64_t)(j0 + j) * gB.piece_len;
                if (UPLINK_ENC_OUT_OK(a, qa, gA, 22)) st16<true>(qa, rA[i].x, rA[i].y, rA[i].z, rA[i].w);
                if (UPLINK_ENC_OUT_OK(a, qb, gB, 22)) st16<true>(qb, rB[i].x, rB[i].y, rB[i].z, rB[i].w);
            }
        }
    };
    // loader: item ch in slot sl from raw bytes to bit planes, in place; the raw
    // bytes are kept in rA / rB for their stores one item later
    auto slice = [&](int sl, int ch, u32x4 *rA, u32x4 *rB) {
        const int j0 = ch * KC, jn = K - j0 < KC ? K - j0 : KC;
        u32x4 *slot = ring + sl * (SLOT / 16);
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int j = lw + NL * i;
            if (j < jn) {
                const u32x4 A4 = slot[j * 128 + lane], B4 = slot[j * 128 + 64 + lane];
                if constexpr (COPY) {
                    rA[i] = A4;
                    rB[i] = B4;
                }
                uint32_t w[8] = {A4.x, A4.y, A4.z, A4.w, B4.x, B4.y, B4.z, B4.w};
                bitslice8(w);
                slot[j * 128 + lane] = (u32x4){w[0], w[1], w[2], w[3]};
                slot[j * 128 + 64 + lane] = (u32x4){w[4], w[5], w[6], w[7]};
            }
        }
    };
    // (uniform: the map is read with it)
    auto tile_of = [&](int item) -> int64_t { return __builtin_amdgcn_readfirstlane(s_q[(item / NCH) & 7]); };

    if (taker)
#pragma unroll
        for (int m = 0; m < K0; m++) s_q[m] = take(m);
    lds_barrier();
    if (loader) {
        // item 0 in flight, then bit-sliced
        const int64_t t0 = tile_of(0);
        if (t0 < P) {
            issue(0, t0, 0);
            wait_vm(0);
            // (item 0's copy-through stores at once: nothing of the loader's is
            // live across the barrier below)
            u32x4 rA0[COPY ? PER : 1], rB0[COPY ? PER : 1];
            slice(0, 0, rA0, rB0);
            if constexpr (COPY) copy_out(t0, 0, rA0, rB0);
        }
    }
    lds_barrier();
    if (loader) {
        // the raw bytes of the item sliced last (from item 1 on), its tile and chunk
        [[maybe_unused]] u32x4 rawA[COPY ? PER : 1], rawB[COPY ? PER : 1];
        [[maybe_unused]] int64_t raw_t = 0;
        [[maybe_unused]] int raw_ch = 0;
        for (int i = 0;; i++) {
            if (tile_of(i) >= P) break;
            const int64_t u1 = tile_of(i + 1);
            if (u1 < P) issue((i + 1) % kSlots, u1, (i + 1) % NCH);
            // item i's copy-through stores, behind item i+1's DMAs
            if constexpr (COPY)
                if (i > 0) copy_out(raw_t, raw_ch, rawA, rawB);
            if (u1 < P) {
                // this wave's VMEM ops issued after item i+1's DMAs: item i's
                // copy-through stores (from item 1 on); completion is in order, so
                // waiting down to that many means item i+1 has landed
                int after = 0;
                if constexpr (COPY && kCountStores)
                    if (i > 0) after += ops_of(i % NCH);
                wait_vm(after);
                slice((i + 1) % kSlots, (i + 1) % NCH, rawA, rawB);
                raw_t = u1;
                raw_ch = (i + 1) % NCH;
            }
            lds_barrier();
        }
        return;
    }
    // compute waves: per tile, the chunks in order with a barrier after each
    uint32_t acc[OPW][8];
    const int w_rbase = rbase_of(R, NC, wave), w_rows = rows_of(R, NC, wave);
    for (int m = 0;; m++) {
        const int64_t ti = tile_of(m * NCH);
        if (ti >= P) break;
#pragma unroll
        for (int o = 0; o < OPW; o++)
#pragma unroll
            for (int p = 0; p < 8; p++) acc[o][p] = 0;
        static_for<NCH>([&]<int C>() __attribute__((always_inline)) {
            const int i = m * NCH + C;
            // the tile of item i+A+1 onwards (when one starts there): its queue atomic
            // returns during this item's multiply and is published before the barrier
            int pend_m = -1;
            int32_t pending = 0;
            if (taker && (i + A + 1) % NCH == 0 && (i + A + 1) / NCH >= K0) {
                pend_m = (i + A + 1) / NCH;
                pending = take(pend_m);
            }
            constexpr int J0 = C * KC, JN = K - J0 < KC ? K - J0 : KC;
            const u32x4 *slot = ring + (i % kSlots) * (SLOT / 16);
            auto hook = [&]<int JJ>() __attribute__((always_inline)) {};
            static_for<NC>([&]<int W>() __attribute__((always_inline)) {
                if (wave == W) compute_chunk<K, N, NC, OPW, W, J0, JN, 0>(slot, lane, acc, hook);
            });
            if (pend_m >= 0) s_q[pend_m & 7] = pending;
            if constexpr (C == NCH - 1) {
                const BlockGeo gA = block_geo<K, ROWS>(a, ti, lane), gB = block_geo<K, ROWS>(a, ti + P, lane);
                static_for<OPW>([&]<int O>() {
                    if (O < w_rows) {
                        uint32_t w[8];
#pragma unroll
                        for (int p = 0; p < 8; p++) w[p] = acc[O][p];
                        unbitslice8(w);
                        const int row = ROW0 + w_rbase + O;
                        uint8_t *qa = gA.out + (int64_t)row * gA.piece_len, *qb = gB.out + (int64_t)row * gB.piece_len;
                        if (gA.v && UPLINK_ENC_OUT_OK(a, qa, gA, 23)) st16<true>(qa, w[0], w[1], w[2], w[3]);
                        if (gB.v && UPLINK_ENC_OUT_OK(a, qb, gB, 23)) st16<true>(qb, w[4], w[5], w[6], w[7]);
                    }
                });
            }
            lds_barrier();
        });
    }
    // The launch's last workgroup to finish zeroes the queue for the next launch
    // that gets it and tells the host through the slot's completion word (encode_body).
    if (taker && a.queue) {
        if (atomicAdd(a.queue + kQueueDoneWord, 1u) == gridDim.x - 1) {
            atomicExch(a.queue, 0u);
            atomicExch(a.queue + kQueueDoneWord, 0u);
            if (a.queue_host_done)
                __hip_atomic_store(a.queue_host_done, a.queue_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int K, int N, int NC, int NL, bool COPY>
__global__ __launch_bounds__((NC + NL) * 64, UPLINK_ENC_WGS > 1 ? (NC + NL) * UPLINK_ENC_WGS / 4 : 1) void rs_encode_sized(
    const EncSizedArgs a) {
    encode_sized_body<K, N, NC, NL, COPY>(a);
}

#undef UPLINK_ENC_IN_OK
#undef UPLINK_ENC_OUT_OK
#undef UPLINK_ENC_IN_LO

}  // namespace enc
}  // namespace uplink_ec
