// Segment repair (rs_repair.hpp): piece t of a segment from its k basis shares
// S.  G is the Lagrange basis on the points x_0 = 0, x_i = alpha^(i-1)
// (gf256_field.hpp), so piece_t = sum over p of L^S_p(x_t) * piece_{s_p}: the
// closed form the share-set decode evaluates at a missing data position
// (rs_sets.hip), taken at any piece's point.  The host solves the rows
// (ec_repair.cpp); here:
//
//  rs_repair_prep: one workgroup per segment copies its descriptor from the
//      host's staging to device memory and writes the rows' jump-table leaf
//      addresses from the staged coefficient bytes (already in table order).
//  rs_repair<NW>: rs_matmul_dma<NW, 1, false> (rs_kernels.hip) with a
//      descriptor per segment as rs_matmul_sets has, for pieces in and pieces
//      out: a lane's two 16-byte chunks sit at the same offset q*16 of every
//      input and output, nothing is copied through, and NW = 8 takes up to 64
//      rows in one pass over the inputs.  Rows from nstore on are syndrome rows
//      (the share check): OR-reduced over the valid columns, never stored.
#include <hip/hip_runtime.h>

#include "gf256_field.hpp"
#include "rs_device.hpp"
#include "rs_repair.hpp"

namespace uplink_ec {
namespace {

using namespace dev;

__constant__ GfTables c_gf = make_gf_tables();

constexpr int kRows = 8;  // accumulator rows per wave (jt_inputs)

__host__ __device__ __forceinline__ void rows_of(int pass, int npass, int nout, int nw, int g, int &rbase, int &cnt) {
    const int p0 = pass * nout / npass, prow = (pass + 1) * nout / npass - p0;
    rbase = p0 + g * prow / nw;
    cnt = p0 + (g + 1) * prow / nw - rbase;
}

__host__ __device__ __forceinline__ int npass_of(int nout, int nw) {
    return nout > 0 ? (nout + nw * kRows - 1) / (nw * kRows) : 1;
}

__global__ __launch_bounds__(256) void rs_repair_prep(const RepairStage *stage, RepairDesc *desc, uint64_t jt_base) {
    const RepairStage *st = stage + blockIdx.x;
    const int tid = threadIdx.x;
    {
        const uint64_t *src = (const uint64_t *)&st->d;
        uint64_t *dst = (uint64_t *)(desc + blockIdx.x);
        for (int i = tid; i < (int)(sizeof(RepairDesc) / 8); i += blockDim.x) dst[i] = src[i];
    }
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

// checked build: an access outside [lo, lo + len) is skipped and its site
// recorded (as rs_tile.hpp in_range does for a launch's ranges, here for the
// segment's own share or output)
__device__ __forceinline__ bool in_span(const RepairArgs &a, const uint8_t *p, const uint8_t *lo, int64_t len, int site) {
#ifdef UPLINK_EC_CHECKED
    if (p >= lo && p + 16 <= lo + len) return true;
    if (a.chk_flag) atomicCAS(a.chk_flag, 0u, (uint32_t)site);
    return false;
#else
    (void)a, (void)p, (void)lo, (void)len, (void)site;
    return true;
#endif
}

// read through the constant address space: uniform loads become scalar loads
// (the jump-table body needs its leaf-table address in SGPRs)
typedef const __attribute__((address_space(4))) RepairDesc ConstDesc;

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_repair(const RepairArgs a) {
    constexpr int JC = 2 * NW, PER = 2, OPW = kRows, SLOT = JC * 2048;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    u32x4 *ring = (u32x4 *)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int group = (wave + (int)(blockIdx.x % NW)) % NW;
    const uint32_t ring_addr = (uint32_t)(uintptr_t)smem;
    const int64_t tile = blockIdx.x;
    const int64_t seg = tile / a.tiles_per_seg;
    ConstDesc *d = (ConstDesc *)(a.desc + seg);
    const int nin = d->nin, nout = d->nout, nstore = d->nstore;
    if (nin <= 0 || nout <= 0) return;
    // the tile's two chunks of 16 byte columns per lane; pieces in, pieces out: the same offset
    const int64_t qA = (tile - seg * a.tiles_per_seg) * kTileChunks + lane, qB = qA + 64;
    const bool vA = qA < a.chunks_per_seg, vB = qB < a.chunks_per_seg;
    // a lane past the end of the piece reads column 0 (never stored, masked out of the check)
    const int64_t iA = vA ? qA * 16 : 0, iB = vB ? qB * 16 : 0;
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
                if (!in_span(a, pa, p, a.piece_len, 10)) pa = p;
                if (!in_span(a, pb, p, a.piece_len, 10)) pb = p;
                const uint32_t dst = __builtin_amdgcn_readfirstlane(d0 + (uint32_t)(j * 2048));
                dma_1k(pa, dst);
                dma_1k(pb, dst + 1024);
            }
        }
    };
    uint32_t bad = 0;
    for (int pass = 0; pass < npass; pass++) {
        int rbase, cnt;
        rows_of(pass, npass, nout, NW, group, rbase, cnt);
        issue(0);
        u32x8 acc[OPW];
#pragma unroll
        for (int o = 0; o < OPW; o++) acc[o] = (u32x8){0, 0, 0, 0, 0, 0, 0, 0};
        for (int ch = 0; ch < nchunks; ch++) {
            // one chunk ahead and nothing copied through: this wave's only VMEM
            // operations in flight are chunk ch's DMAs (and the last pass's stores)
            wait_vm(0);
            const int j0 = ch * CH;
            u32x4 *slot = ring + (ch & 1) * (SLOT / 16);
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int j = wave + NW * i;
                if (i < owned(ch)) {
                    const u32x4 A4 = slot[j * 128 + lane], B4 = slot[j * 128 + 64 + lane];
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
                          d->tgt + ((int64_t)(pass * nin + j0) * NW + group) * OPW, (uint32_t)(NW * OPW * 8),
                          (uint32_t)(OPW - cnt), (uint32_t)jn);
            }
        }
        uint32_t rows[OPW][8];
#pragma unroll
        for (int o = 0; o < OPW; o++)
#pragma unroll
            for (int p = 0; p < 8; p++) rows[o][p] = acc[o][p];
        // syndrome rows: a non-basis share predicted from the basis, plus the share
        // itself (coefficient 1 on its own row); any set bit of a valid column is a
        // difference (plane bits 0-3 of each byte are chunk A, bits 4-7 chunk B)
        if (rbase + cnt > nstore) {
            uint32_t any = 0;
#pragma unroll
            for (int o = 0; o < OPW; o++)
                if (o < cnt && rbase + o >= nstore)
#pragma unroll
                    for (int p = 0; p < 8; p++) any |= rows[o][p];
            bad |= any & ((vA ? 0x0F0F0F0Fu : 0u) | (vB ? 0xF0F0F0F0u : 0u));
        }
        static_for<OPW>([&]<int O>() {
            if (O < cnt && rbase + O < nstore) {
                uint32_t w[8];
#pragma unroll
                for (int p = 0; p < 8; p++) w[p] = rows[O][p];
                unbitslice8(w);
                uint8_t *p = d->out[rbase + O];
                if (vA && in_span(a, p + qA * 16, p, a.piece_len, 11)) st16<true>(p + qA * 16, w[0], w[1], w[2], w[3]);
                if (vB && in_span(a, p + qB * 16, p, a.piece_len, 11)) st16<true>(p + qB * 16, w[4], w[5], w[6], w[7]);
            }
        });
        // the slot the next pass's first DMAs go to may still be read by a wave's multiply
        lds_barrier();
    }
    if (nout > nstore) {
        int32_t *st = d->status;
        if (__ballot(bad != 0) != 0 && lane == 0 && st) atomicOr(st, 1);
    }
}

// The byte path's share check: row r of the launch's matrix, computed as
// rs_matmul_bytes computes it, against the share at out_off[r].
__global__ __launch_bounds__(256) void rs_repair_check_bytes(const RsArgs a) {
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ int s_bad;
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = c_gf.exp[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = c_gf.log[i];
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int64_t cols = a.nstripes * a.ess;
    bool bad = false;
    for (int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; col < cols; col += (int64_t)gridDim.x * blockDim.x) {
        for (int r = 0; r < a.nout; r++) {
            uint8_t acc = 0;
            for (int j = 0; j < a.nin; j++) {
                const uint8_t x = a.in_base[a.in_off[j] + col];
                const uint8_t cv = a.coef[(int64_t)j * a.coef_ld + r];
                if (x && cv) acc ^= s_exp[s_log[x] + s_log[cv]];
            }
            bad = bad || acc != a.out_base[a.out_off[r] + col];
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicOr(a.zero_check, 1u);
}

}  // namespace

int repair_waves(int rows) { return rows <= 14 ? 2 : rows <= 24 ? 3 : rows <= 32 ? 4 : 8; }

int repair_npass(int nout, int nw) { return npass_of(nout, nw); }

void repair_rows_of(int pass, int npass, int nout, int nw, int g, int &rbase, int &cnt) {
    rows_of(pass, npass, nout, nw, g, rbase, cnt);
}

size_t repair_tgt_entries(int nin, int rows, int nw) {
    return ((size_t)npass_of(rows, nw) * nin * nw * kRows + 15) & ~(size_t)15;
}

int64_t repair_max_tiles(int nw) { return (int64_t)(0xFFFFFFFFu / (unsigned)(nw * 64)); }

hipError_t launch_repair_prep(const RepairStage *stage, RepairDesc *desc, int nseg, uint64_t jt_base, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_repair_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base);
    return hipGetLastError();
}

hipError_t launch_repair(const RepairArgs &a, int nw, hipStream_t s) {
    if (a.total_tiles <= 0) return hipSuccess;
    if (a.total_tiles > repair_max_tiles(nw)) return hipErrorInvalidValue;  // one workgroup per tile
    const dim3 grid((unsigned)a.total_tiles);
    // two slots of 2 * NW inputs, 2 KiB each: 64 KiB on 8 waves, what a launch gets by default
    switch (nw) {
    case 2: hipLaunchKernelGGL(rs_repair<2>, grid, dim3(2 * 64), (size_t)2 * 4 * 2048, s, a); break;
    case 3: hipLaunchKernelGGL(rs_repair<3>, grid, dim3(3 * 64), (size_t)2 * 6 * 2048, s, a); break;
    case 4: hipLaunchKernelGGL(rs_repair<4>, grid, dim3(4 * 64), (size_t)2 * 8 * 2048, s, a); break;
    case 8: hipLaunchKernelGGL(rs_repair<8>, grid, dim3(8 * 64), (size_t)2 * 16 * 2048, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_repair_check_bytes(const RsArgs &a, hipStream_t s) {
    const int64_t cols = a.nstripes * a.ess;
    if (cols <= 0 || a.nout <= 0) return hipSuccess;
    int64_t blocks = (cols + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rs_repair_check_bytes, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace uplink_ec
