// The tile body of the share-set kernels -- rs_matmul_sets, rs_sets_one
// (rs_sets.hip), rs_matmul_sized (rs_sized.hip), rs_repair (rs_repair.hip) --
// and what their prep kernels and launchers share.
//
// share_tile<NW, Geom> is rs_matmul_dma<NW, 1, false> (rs_kernels.hip) with the
// per-launch matrix replaced by a descriptor per segment: one workgroup per
// 2048-column tile, the inputs staged by LDS-DMA into a ring of two slots one
// chunk ahead, bit-sliced in place, multiplied by the jump-table body
// (jt_inputs), the rows unloaded, syndrome rows OR-reduced, the others
// transposed back and stored.  Geom, a struct of force-inlined members that the
// kernel's wrapper fills for its workgroup, says what differs between kernels:
//
//   d                       the segment's descriptor through the constant address space
//                           (in[], tgt, nin, nout: uniform loads from there are scalar
//                           loads, and jt_inputs needs its leaf-table address in SGPRs)
//   skip(nin, nout)         nothing to do for this workgroup
//   cols(lane)              the lane's two chunks of 16 byte columns: sets vA, vB (inside
//                           the segment), iA, iB (byte offsets in an input), oA, oB (in an output)
//   in_ok(p, share)         checked build: p's 16 bytes lie inside the input `share`
//   kCopy, copy_off(j),     basis data shares copied through to out_base() + copy_off(j)
//   out_base()              on pass 0 (kCopy false: neither is asked for)
//   row_out(r)              where stored row r's columns start
//   out_ok(p, row)          checked build: p's 16 bytes lie inside the output of `row`
//   stored(rbase, cnt)      rows below this are stored, those from it on are syndrome rows
//   checks(rbase, cnt, nst) the group has syndrome rows in this pass
//   report(any, lane)       their OR over the lane's valid columns, per pass
//   finish(lane)            after the last pass
//   kOwnTable,              rs_sets_one: the workgroup writes the leaf table itself while its
//   write_table<NW>(...)    first chunk's loads are in flight (rs_sets.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "rs_device.hpp"
#include "rs_rows.hpp"

namespace uplink_ec {
namespace dev {

// checked build: an access outside [lo, lo + len) -- the segment's own share or
// output -- is skipped and its site recorded (as rs_tile.hpp in_range does for a
// launch's ranges)
template <class Args>
__device__ __forceinline__ bool in_span(const Args &a, const uint8_t *p, const uint8_t *lo, int64_t len, int site) {
#ifdef UPLINK_EC_CHECKED
    if (p >= lo && p + 16 <= lo + len) return true;
    if (a.chk_flag) atomicCAS(a.chk_flag, 0u, (uint32_t)site);
    return false;
#else
    (void)a, (void)p, (void)lo, (void)len, (void)site;
    return true;
#endif
}

// prep kernels: the segment's descriptor from the host's staging to device memory at once (one
// round trip over the bus, or the kernel's arguments)
template <class Desc>
__device__ __forceinline__ void copy_desc(const Desc *src, Desc *dst) {
    static_assert(sizeof(Desc) % 8 == 0, "copied as 8-byte words");
    const uint64_t *s = (const uint64_t *)src;
    uint64_t *d = (uint64_t *)dst;
    for (int i = threadIdx.x; i < (int)(sizeof(Desc) / 8); i += blockDim.x) d[i] = s[i];
}

// prep kernels: the staged coefficient bytes (already in table order, pack_rows) into leaf
// addresses; 16 coefficients per load over the bus, 16 leaf addresses out
__device__ __forceinline__ void write_leaves(const uint8_t *coef, int64_t entries, uint64_t *tgt, uint64_t jt_base) {
    const uint4 *cf = (const uint4 *)coef;
    const int64_t n16 = entries / 16;
    for (int64_t i = threadIdx.x; i < n16; i += blockDim.x) {
        const uint4 v = cf[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++)
            tgt[i * 16 + b] = jt_base + (uint64_t)((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) * RS_JT_SLOT;
    }
}

// What the geometries of rs_sets.hip and rs_sized.hip share: shares in, a
// stripe-major segment [stripe][k][ess] out, Decode's syndrome counter.  D: the
// descriptor (out, copy_off, out_off, zero_check, nstore).
template <class D>
struct StripeGeom {
    static constexpr bool kCopy = true;
    D *d;
    bool vA, vB;
    int64_t iA, iB, oA, oB;
    uint8_t *out;
    uint32_t *zc;

    // chunk qA of the segment's `chunks`, and the one 64 on: stripe s, chunk t of the share's cps
    __device__ __forceinline__ void stripe_cols(int64_t qA, int64_t chunks, int cps_, int ess, int k) {
        const int64_t qB = qA + 64;
        vA = qA < chunks, vB = qB < chunks;
        const uint32_t cps = (uint32_t)cps_;
        // (chunks fits 32 bits, so a valid lane's index does; an invalid lane's quotient is not used)
        const uint32_t sA = (uint32_t)qA / cps, tA = (uint32_t)qA - sA * cps;
        const uint32_t sB = (uint32_t)qB / cps, tB = (uint32_t)qB - sB * cps;
        // a lane past the end of the segment reads the segment's column 0 (never stored)
        iA = vA ? (int64_t)sA * ess + tA * 16 : 0, iB = vB ? (int64_t)sB * ess + tB * 16 : 0;
        oA = (int64_t)sA * k * ess + tA * 16, oB = (int64_t)sB * k * ess + tB * 16;
        out = d->out;
    }
    __device__ __forceinline__ int copy_off(int j) const { return d->copy_off[j]; }
    __device__ __forceinline__ uint8_t *out_base() const { return out; }
    __device__ __forceinline__ uint8_t *row_out(int r) const { return out + d->out_off[r]; }
    // with a counter (Decode), rows from nstore on are syndrome rows, and every wave that
    // finds a difference in a pass adds 1
    __device__ __forceinline__ int stored(int rbase, int cnt) {
        zc = d->zero_check;
        return zc ? d->nstore : rbase + cnt;
    }
    __device__ __forceinline__ bool checks(int, int, int) const { return zc != nullptr; }
    __device__ __forceinline__ void report(uint32_t any, int lane) const {
        if (__ballot(any != 0) != 0 && lane == 0) atomicAdd(zc, 1u);
    }
    __device__ __forceinline__ void finish(int) const {}
};

template <int NW, class Geom>
__device__ __forceinline__ void share_tile(Geom &G) {
    constexpr int JC = 2 * NW, PER = 2, OPW = kRows, SLOT = JC * 2048;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    u32x4 *ring = (u32x4 *)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int group = (wave + (int)(blockIdx.x % NW)) % NW;
    const uint32_t ring_addr = (uint32_t)(uintptr_t)smem;
    const int nin = G.d->nin, nout = G.d->nout;
    if (G.skip(nin, nout)) return;
    G.cols(lane);
    const bool vA = G.vA, vB = G.vB;
    const int nchunks = (nin + JC - 1) / JC;
    const int CH = (nin + nchunks - 1) / nchunks;
    const int npass = npass_of(nout, NW);
    auto owned = [&](int ch) -> int {
        const int jn = nin - ch * CH < CH ? nin - ch * CH : CH;
        return wave < jn ? (jn - wave + NW - 1) / NW : 0;
    };
    auto issue = [&](int ch) {
        const uint32_t d0 = ring_addr + (uint32_t)((ch & 1) * SLOT);
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int j = wave + NW * i;
            if (i < owned(ch)) {
                const uint8_t *p = G.d->in[ch * CH + j];
                const uint8_t *pa = p + G.iA, *pb = p + G.iB;
                if (!G.in_ok(pa, p)) pa = p;
                if (!G.in_ok(pb, p)) pb = p;
                const uint32_t dst = __builtin_amdgcn_readfirstlane(d0 + (uint32_t)(j * 2048));
                dma_1k(pa, dst);
                dma_1k(pb, dst + 1024);
            }
        }
    };
    if constexpr (Geom::kOwnTable) {
        issue(0);
        G.template write_table<NW>(npass, nin, nout);
    }
    for (int pass = 0; pass < npass; pass++) {
        int rbase, cnt;
        rows_of(pass, npass, nout, NW, group, rbase, cnt);
        if (!Geom::kOwnTable || pass > 0) issue(0);
        u32x8 acc[OPW];
#pragma unroll
        for (int o = 0; o < OPW; o++) acc[o] = (u32x8){0, 0, 0, 0, 0, 0, 0, 0};
        for (int ch = 0; ch < nchunks; ch++) {
            // one chunk ahead: this wave's only VMEM operations in flight are chunk ch's
            // DMAs (and the stores of the last pass or of the copy-through)
            wait_vm(0);
            const int j0 = ch * CH;
            u32x4 *slot = ring + (ch & 1) * (SLOT / 16);
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int j = wave + NW * i;
                if (i < owned(ch)) {
                    const u32x4 A4 = slot[j * 128 + lane], B4 = slot[j * 128 + 64 + lane];
                    if constexpr (Geom::kCopy) {
                        const int co = G.copy_off(j0 + j);
                        if (pass == 0 && co >= 0) {
                            uint8_t *p = G.out_base() + co;
                            if (vA && G.out_ok(p + G.oA, p)) st16<true>(p + G.oA, A4.x, A4.y, A4.z, A4.w);
                            if (vB && G.out_ok(p + G.oB, p)) st16<true>(p + G.oB, B4.x, B4.y, B4.z, B4.w);
                        }
                    }
                    uint32_t w[8] = {A4.x, A4.y, A4.z, A4.w, B4.x, B4.y, B4.z, B4.w};
                    bitslice8(w);
                    // in place, in the wide layout jt_inputs reads (a lane's planes where its bytes were)
                    slot[j * 128 + lane] = (u32x4){w[0], w[1], w[2], w[3]};
                    slot[j * 128 + 64 + lane] = (u32x4){w[4], w[5], w[6], w[7]};
                }
            }
            lds_barrier();
            // chunk ch+1 into the slot chunk ch-1 left (every wave is past its multiply)
            if (ch + 1 < nchunks) issue(ch + 1);
            if (cnt > 0) {
                const int jn = nin - j0 < CH ? nin - j0 : CH;
                jt_inputs(acc, ring_addr + (uint32_t)((ch & 1) * SLOT) + (uint32_t)lane * 16,
                          G.d->tgt + ((int64_t)(pass * nin + j0) * NW + group) * OPW, (uint32_t)(NW * OPW * 8),
                          (uint32_t)(OPW - cnt), (uint32_t)jn);
            }
        }
        uint32_t rows[OPW][8];
#pragma unroll
        for (int o = 0; o < OPW; o++)
#pragma unroll
            for (int p = 0; p < 8; p++) rows[o][p] = acc[o][p];
        // rows from nst on are syndrome rows: a non-basis share predicted from the basis, plus
        // the share itself (coefficient 1 on its own row); any set bit of a valid column is a
        // difference (plane bits 0-3 of each byte are chunk A, bits 4-7 chunk B)
        const int nst = G.stored(rbase, cnt);
        if (G.checks(rbase, cnt, nst)) {
            uint32_t any = 0;
#pragma unroll
            for (int o = 0; o < OPW; o++)
                if (o < cnt && rbase + o >= nst)
#pragma unroll
                    for (int p = 0; p < 8; p++) any |= rows[o][p];
            any &= (vA ? 0x0F0F0F0Fu : 0u) | (vB ? 0xF0F0F0F0u : 0u);
            G.report(any, lane);
        }
        static_for<OPW>([&]<int O>() {
            if (O < cnt && rbase + O < nst) {
                uint32_t w[8];
#pragma unroll
                for (int p = 0; p < 8; p++) w[p] = rows[O][p];
                unbitslice8(w);
                uint8_t *p = G.row_out(rbase + O);
                if (vA && G.out_ok(p + G.oA, p)) st16<true>(p + G.oA, w[0], w[1], w[2], w[3]);
                if (vB && G.out_ok(p + G.oB, p)) st16<true>(p + G.oB, w[4], w[5], w[6], w[7]);
            }
        });
        // the slot the next pass's first DMAs go to may still be read by a wave's multiply
        lds_barrier();
    }
    G.finish(lane);
}

// One workgroup of nw waves per tile on the kernel's instantiation for nw (null: none), with the
// ring's two slots of 2 * nw inputs, 2 KiB each (64 KiB on 8 waves, what a launch gets by default).
template <class Args>
inline hipError_t launch_share_tile(const Args &a, int64_t tiles, int nw, hipStream_t s, void (*k2)(Args),
                                    void (*k3)(Args), void (*k4)(Args), void (*k8)(Args) = nullptr) {
    if (tiles <= 0) return hipSuccess;
    if (tiles > share_max_tiles(nw)) return hipErrorInvalidValue;
    void (*const k)(Args) = nw == 2 ? k2 : nw == 3 ? k3 : nw == 4 ? k4 : nw == 8 ? k8 : nullptr;
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(nw * 64), (size_t)2 * 2 * nw * 2048, s, a);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace uplink_ec
