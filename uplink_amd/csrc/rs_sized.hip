// Share-set Rebuild / Decode of segments of different sizes (rs_sized.hpp).
//
//  rs_sized_prep: one workgroup per segment copies its descriptor from the
//      host's staging to device memory, writes the rows' jump-table leaf
//      addresses from the staged coefficient bytes (already in table order),
//      fills the segment's range of its class's tile map with the segment's
//      position and zeroes its syndrome counter.
//  rs_matmul_sized<NW>: the tile body of rs_matmul_sets (rs_sets.hip) restated
//      with per-segment geometry: the workgroup reads its map entry with one
//      uniform load, then the descriptor through the constant address space;
//      the ragged last tile is masked by the segment's own chunk count, output
//      offsets are taken within the segment's own stripes.
#include <hip/hip_runtime.h>

#include "rs_device.hpp"
#include "rs_sized.hpp"

namespace uplink_ec {
namespace {

using namespace dev;

constexpr int kRows = 8;  // accumulator rows per wave (jt_inputs)

__host__ __device__ __forceinline__ void rows_of(int pass, int npass, int nout, int nw, int g, int &rbase, int &cnt) {
    const int p0 = pass * nout / npass, prow = (pass + 1) * nout / npass - p0;
    rbase = p0 + g * prow / nw;
    cnt = p0 + (g + 1) * prow / nw - rbase;
}

__host__ __device__ __forceinline__ int npass_of(int nout, int nw) {
    return nout > 0 ? (nout + nw * kRows - 1) / (nw * kRows) : 1;
}

__global__ __launch_bounds__(256) void rs_sized_prep(const SizedStage *stage, SizedDesc *desc, uint64_t jt_base) {
    const SizedStage *st = stage + blockIdx.x;
    const int tid = threadIdx.x;
    {
        const uint64_t *src = (const uint64_t *)&st->d;
        uint64_t *dst = (uint64_t *)(desc + blockIdx.x);
        for (int i = tid; i < (int)(sizeof(SizedDesc) / 8); i += blockDim.x) dst[i] = src[i];
    }
    if (tid == 0) {
        uint32_t *zc = st->d.zero_check;
        if (zc) *zc = 0u;
    }
    // the segment's tiles of its class's map: all this segment
    uint32_t *map = st->map;
    const int64_t ntiles = st->ntiles;
    for (int64_t i = tid; i < ntiles; i += blockDim.x) map[i] = blockIdx.x;
    // 16 coefficients per load over the bus, 16 leaf addresses out
    const uint4 *cf = (const uint4 *)st->coef;
    uint64_t *tgt = st->d.tgt;
    const int64_t n16 = st->entries / 16;
    for (int64_t i = tid; i < n16; i += blockDim.x) {
        const uint4 v = cf[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++)
            tgt[i * 16 + b] = jt_base + (uint64_t)((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) * RS_JT_SLOT;
    }
}

// checked build: an access outside [lo, lo + len) -- the segment's own share or
// output -- is skipped and its site recorded (as rs_sets.hip in_span)
__device__ __forceinline__ bool in_span(const SizedArgs &a, const uint8_t *p, const uint8_t *lo, int64_t len, int site) {
#ifdef UPLINK_EC_CHECKED
    if (p >= lo && p + 16 <= lo + len) return true;
    if (a.chk_flag) atomicCAS(a.chk_flag, 0u, (uint32_t)site);
    return false;
#else
    (void)a, (void)p, (void)lo, (void)len, (void)site;
    return true;
#endif
}

// The map and the descriptors are read through the constant address space: the
// kernel never writes them, and uniform loads from there are scalar loads (the
// jump-table body needs its leaf-table address in SGPRs).
typedef const __attribute__((address_space(4))) SizedDesc ConstDesc;
typedef const __attribute__((address_space(4))) uint32_t ConstMap;

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_matmul_sized(const SizedArgs a) {
    constexpr int JC = 2 * NW, PER = 2, OPW = kRows, SLOT = JC * 2048;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    u32x4 *ring = (u32x4 *)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int group = (wave + (int)(blockIdx.x % NW)) % NW;
    const uint32_t ring_addr = (uint32_t)(uintptr_t)smem;
    // the workgroup's tile of the class, its segment, and the tile within the segment
    const int64_t ctile = a.tile_base + blockIdx.x;
    const uint32_t q = __builtin_amdgcn_readfirstlane(((ConstMap *)a.map)[ctile]);
    ConstDesc *d = (ConstDesc *)(a.desc + q);
    const int nin = d->nin, nout = d->nout;
    const int64_t chunks = d->chunks, piece_len = d->piece_len, spad = d->spad;
    const int64_t tile = ctile - d->tile0;
    if (nin <= 0 || tile < 0) return;
    // the tile's two chunks of 16 byte columns per lane, masked by the segment's own chunk count
    const int64_t qA = tile * kTileChunks + lane, qB = qA + 64;
    const bool vA = qA < chunks, vB = qB < chunks;
    const uint32_t cps = (uint32_t)a.cps;
    // (chunks fits 32 bits, so a valid lane's index does; an invalid lane's quotient is not used)
    const uint32_t sA = (uint32_t)qA / cps, tA = (uint32_t)qA - sA * cps;
    const uint32_t sB = (uint32_t)qB / cps, tB = (uint32_t)qB - sB * cps;
    // a lane past the end of the segment reads the segment's column 0 (never stored)
    const int64_t iA = vA ? (int64_t)sA * a.ess + tA * 16 : 0, iB = vB ? (int64_t)sB * a.ess + tB * 16 : 0;
    const int64_t oA = (int64_t)sA * a.k * a.ess + tA * 16, oB = (int64_t)sB * a.k * a.ess + tB * 16;
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
                const uint8_t *p = d->in[ch * CH + j];
                const uint8_t *pa = p + iA, *pb = p + iB;
                if (!in_span(a, pa, p, piece_len, 12)) pa = p;
                if (!in_span(a, pb, p, piece_len, 12)) pb = p;
                const uint32_t dst = __builtin_amdgcn_readfirstlane(d0 + (uint32_t)(j * 2048));
                dma_1k(pa, dst);
                dma_1k(pb, dst + 1024);
            }
        }
    };
    uint8_t *out = d->out;
    for (int pass = 0; pass < npass; pass++) {
        int rbase, cnt;
        rows_of(pass, npass, nout, NW, group, rbase, cnt);
        issue(0);
        u32x8 acc[OPW];
#pragma unroll
        for (int o = 0; o < OPW; o++) acc[o] = (u32x8){0, 0, 0, 0, 0, 0, 0, 0};
        for (int ch = 0; ch < nchunks; ch++) {
            wait_vm(0);
            const int j0 = ch * CH;
            u32x4 *slot = ring + (ch & 1) * (SLOT / 16);
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int j = wave + NW * i;
                if (i < owned(ch)) {
                    const u32x4 A4 = slot[j * 128 + lane], B4 = slot[j * 128 + 64 + lane];
                    const int co = d->copy_off[j0 + j];
                    if (pass == 0 && co >= 0) {
                        uint8_t *p = out + co;
                        if (vA && in_span(a, p + oA, out, spad, 13)) st16<true>(p + oA, A4.x, A4.y, A4.z, A4.w);
                        if (vB && in_span(a, p + oB, out, spad, 13)) st16<true>(p + oB, B4.x, B4.y, B4.z, B4.w);
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
                          d->tgt + ((pass * nin + j0) * NW + group) * OPW, (uint32_t)(NW * OPW * 8),
                          (uint32_t)(OPW - cnt), (uint32_t)jn);
            }
        }
        uint32_t rows[OPW][8];
#pragma unroll
        for (int o = 0; o < OPW; o++)
#pragma unroll
            for (int p = 0; p < 8; p++) rows[o][p] = acc[o][p];
        // rows past nstore are syndrome rows (Decode): a non-basis share predicted from the
        // basis plus the share itself; any set bit of a valid column is a difference (plane
        // bits 0-3 of each byte are chunk A, bits 4-7 chunk B)
        uint32_t *zc = d->zero_check;
        const int nst = zc ? d->nstore : rbase + cnt;
        if (zc) {
            uint32_t any = 0;
#pragma unroll
            for (int o = 0; o < OPW; o++)
                if (o < cnt && rbase + o >= nst)
#pragma unroll
                    for (int p = 0; p < 8; p++) any |= rows[o][p];
            any &= (vA ? 0x0F0F0F0Fu : 0u) | (vB ? 0xF0F0F0F0u : 0u);
            if (__ballot(any != 0) != 0 && lane == 0) atomicAdd(zc, 1u);
        }
        static_for<OPW>([&]<int O>() {
            if (O < cnt && rbase + O < nst) {
                uint32_t w[8];
#pragma unroll
                for (int p = 0; p < 8; p++) w[p] = rows[O][p];
                unbitslice8(w);
                uint8_t *p = out + d->out_off[rbase + O];
                if (vA && in_span(a, p + oA, out, spad, 13)) st16<true>(p + oA, w[0], w[1], w[2], w[3]);
                if (vB && in_span(a, p + oB, out, spad, 13)) st16<true>(p + oB, w[4], w[5], w[6], w[7]);
            }
        });
        // the slot the next pass's first DMAs go to may still be read by a wave's multiply
        lds_barrier();
    }
}

}  // namespace

int sized_npass(int nout, int nw) { return npass_of(nout, nw); }

void sized_rows_of(int pass, int npass, int nout, int nw, int g, int &rbase, int &cnt) {
    rows_of(pass, npass, nout, nw, g, rbase, cnt);
}

size_t sized_tgt_entries(int nin, int rows, int nw) {
    return ((size_t)npass_of(rows, nw) * nin * nw * kRows + 15) & ~(size_t)15;
}

hipError_t launch_sized_prep(const SizedStage *stage, SizedDesc *desc, int nseg, uint64_t jt_base, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_sized_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base);
    return hipGetLastError();
}

hipError_t launch_matmul_sized(const SizedArgs &a, int nw, hipStream_t s) {
    if (a.total_tiles <= 0) return hipSuccess;
    if (a.total_tiles > (int64_t)(0xFFFFFFFFu / (unsigned)(nw * 64))) return hipErrorInvalidValue;  // one workgroup per tile
    const dim3 grid((unsigned)a.total_tiles);
    // two slots of 2 * NW inputs, 2 KiB each
    switch (nw) {
    case 2: hipLaunchKernelGGL(rs_matmul_sized<2>, grid, dim3(2 * 64), (size_t)2 * 4 * 2048, s, a); break;
    case 3: hipLaunchKernelGGL(rs_matmul_sized<3>, grid, dim3(3 * 64), (size_t)2 * 6 * 2048, s, a); break;
    case 4: hipLaunchKernelGGL(rs_matmul_sized<4>, grid, dim3(4 * 64), (size_t)2 * 8 * 2048, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace uplink_ec
