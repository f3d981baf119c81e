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
//  rs_repair<NW>: the share-set tile body (rs_sets_tile.hpp share_tile) for
//      pieces in and pieces out (RepairGeom); NW = 8 takes up to 64 rows in one
//      pass over the inputs.  Rows from nstore on are syndrome rows (the share
//      check): OR-reduced over the valid columns, never stored.
//  rs_repair_sized_prep, rs_repair_sized<NW>: the same for segments of
//      different sizes in one launch (RepairSizedGeom): the prep kernel also
//      fills the segment's range of its class's tile map, and a workgroup finds
//      its segment through that map, as rs_matmul_sized does (rs_sized.hip).
#include <hip/hip_runtime.h>

#include "gf256_field.hpp"
#include "rs_repair.hpp"
#include "rs_sets_tile.hpp"

namespace uplink_ec {
namespace {

using namespace dev;

__constant__ GfTables c_gf = make_gf_tables();

__global__ __launch_bounds__(256) void rs_repair_prep(const RepairStage *stage, RepairDesc *desc, uint64_t jt_base) {
    const RepairStage *st = stage + blockIdx.x;
    copy_desc(&st->d, desc + blockIdx.x);
    write_leaves(st->coef, st->entries, st->d.tgt, jt_base);
}

// read through the constant address space: uniform loads become scalar loads
typedef const __attribute__((address_space(4))) RepairDesc ConstDesc;

// The tile body's geometry (rs_sets_tile.hpp) of a repair launch: pieces in,
// pieces out, so a lane's two chunks sit at the same offset q*16 of every input
// and output; nothing is copied through; a failed share check sets bit 0 of the
// segment's status word once, after the last pass.
struct RepairGeom {
    static constexpr bool kCopy = false, kOwnTable = false;
    const RepairArgs &a;
    ConstDesc *d;
    const int nstore;
    bool vA, vB;
    int64_t iA, iB, oA, oB;
    uint32_t bad = 0;

    __device__ __forceinline__ bool skip(int nin, int nout) const { return nin <= 0 || nout <= 0; }
    __device__ __forceinline__ void cols(int lane) {
        const int64_t tile = blockIdx.x;
        const int64_t seg = tile / a.tiles_per_seg;
        const int64_t qA = (tile - seg * a.tiles_per_seg) * kTileChunks + lane, qB = qA + 64;
        vA = qA < a.chunks_per_seg, vB = qB < a.chunks_per_seg;
        // a lane past the end of the piece reads column 0 (never stored, masked out of the check)
        iA = vA ? qA * 16 : 0, iB = vB ? qB * 16 : 0;
        oA = qA * 16, oB = qB * 16;
    }
    __device__ __forceinline__ bool in_ok(const uint8_t *p, const uint8_t *share) const {
        return in_span(a, p, share, a.piece_len, 10);
    }
    __device__ __forceinline__ bool out_ok(const uint8_t *p, const uint8_t *row) const {
        return in_span(a, p, row, a.piece_len, 11);
    }
    __device__ __forceinline__ uint8_t *row_out(int r) const { return d->out[r]; }
    __device__ __forceinline__ int stored(int, int) const { return nstore; }
    __device__ __forceinline__ bool checks(int rbase, int cnt, int nst) const { return rbase + cnt > nst; }
    __device__ __forceinline__ void report(uint32_t any, int) { bad |= any; }
    __device__ __forceinline__ void finish(int lane) const {
        if (d->nout > nstore) {
            int32_t *st = d->status;
            if (__ballot(bad != 0) != 0 && lane == 0 && st) atomicOr(st, 1);
        }
    }
};

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_repair(const RepairArgs a) {
    ConstDesc *d = (ConstDesc *)(a.desc + blockIdx.x / a.tiles_per_seg);
    RepairGeom G{a, d, d->nstore};
    share_tile<NW>(G);
}

// ---- segments of different sizes (ec_repair_segments_sized) ----

__global__ __launch_bounds__(256) void rs_repair_sized_prep(const RepairSizedStage *stage, RepairSizedDesc *desc,
                                                            uint64_t jt_base) {
    const RepairSizedStage *st = stage + blockIdx.x;
    copy_desc(&st->d, desc + blockIdx.x);
    // the segment's tiles of its class's map: all this segment
    uint32_t *map = st->map;
    const int64_t ntiles = st->ntiles;
    for (int64_t i = threadIdx.x; i < ntiles; i += blockDim.x) map[i] = blockIdx.x;
    write_leaves(st->coef, st->entries, st->d.tgt, jt_base);
}

// The map and the descriptors are read through the constant address space: the
// kernel never writes them, and uniform loads from there are scalar loads.
typedef const __attribute__((address_space(4))) RepairSizedDesc ConstSizedDesc;
typedef const __attribute__((address_space(4))) uint32_t ConstMap;

// RepairGeom with the segment found through the class's map (as SizedGeom finds
// it, rs_sized.hip) and the tile, the ragged end and the extents taken from the
// segment's own descriptor.
struct RepairSizedGeom {
    static constexpr bool kCopy = false, kOwnTable = false;
    const RepairSizedArgs &a;
    ConstSizedDesc *d;
    const int64_t tile;  // the workgroup's tile within its segment
    const int nstore;
    bool vA, vB;
    int64_t iA, iB, oA, oB;
    uint32_t bad = 0;

    // ctile: the workgroup's tile of the class; its segment through the map
    __device__ __forceinline__ RepairSizedGeom(const RepairSizedArgs &a_, int64_t ctile)
        : a(a_),
          d((ConstSizedDesc *)(a_.desc + (uint32_t)__builtin_amdgcn_readfirstlane(((ConstMap *)a_.map)[ctile]))),
          tile(ctile - d->tile0), nstore(d->nstore) {}
    __device__ __forceinline__ bool skip(int nin, int nout) const { return nin <= 0 || nout <= 0 || tile < 0; }
    __device__ __forceinline__ void cols(int lane) {
        const int64_t chunks = d->chunks;
        const int64_t qA = tile * kTileChunks + lane, qB = qA + 64;
        vA = qA < chunks, vB = qB < chunks;
        // a lane past the end of the piece reads column 0 of its own segment's share (never
        // stored, masked out of the check)
        iA = vA ? qA * 16 : 0, iB = vB ? qB * 16 : 0;
        oA = qA * 16, oB = qB * 16;
    }
    __device__ __forceinline__ bool in_ok(const uint8_t *p, const uint8_t *share) const {
        return in_span(a, p, share, d->piece_len, 14);
    }
    __device__ __forceinline__ bool out_ok(const uint8_t *p, const uint8_t *row) const {
        return in_span(a, p, row, d->piece_len, 15);
    }
    __device__ __forceinline__ uint8_t *row_out(int r) const { return d->out[r]; }
    __device__ __forceinline__ int stored(int, int) const { return nstore; }
    __device__ __forceinline__ bool checks(int rbase, int cnt, int nst) const { return rbase + cnt > nst; }
    __device__ __forceinline__ void report(uint32_t any, int) { bad |= any; }
    __device__ __forceinline__ void finish(int lane) const {
        if (d->nout > nstore) {
            int32_t *st = d->status;
            if (__ballot(bad != 0) != 0 && lane == 0 && st) atomicOr(st, 1);
        }
    }
};

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_repair_sized(const RepairSizedArgs a) {
    RepairSizedGeom G(a, a.tile_base + blockIdx.x);
    share_tile<NW>(G);
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

hipError_t launch_repair_prep(const RepairStage *stage, RepairDesc *desc, int nseg, uint64_t jt_base, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_repair_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base);
    return hipGetLastError();
}

hipError_t launch_repair(const RepairArgs &a, int nw, hipStream_t s) {
    return launch_share_tile(a, a.total_tiles, nw, s, rs_repair<2>, rs_repair<3>, rs_repair<4>, rs_repair<8>);
}

hipError_t launch_repair_sized_prep(const RepairSizedStage *stage, RepairSizedDesc *desc, int nseg, uint64_t jt_base,
                                    hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_repair_sized_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base);
    return hipGetLastError();
}

hipError_t launch_repair_sized(const RepairSizedArgs &a, int nw, hipStream_t s) {
    return launch_share_tile(a, a.total_tiles, nw, s, rs_repair_sized<2>, rs_repair_sized<3>, rs_repair_sized<4>,
                             rs_repair_sized<8>);
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
