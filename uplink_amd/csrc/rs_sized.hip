// Share-set Rebuild / Decode of segments of different sizes (rs_sized.hpp).
//
//  rs_sized_prep: one workgroup per segment copies its descriptor from the
//      host's staging to device memory, writes the rows' jump-table leaf
//      addresses from the staged coefficient bytes (already in table order),
//      fills the segment's range of its class's tile map with the segment's
//      position and zeroes its syndrome counter.
//  rs_matmul_sized<NW>: the share-set tile body (rs_sets_tile.hpp share_tile)
//      with per-segment geometry (SizedGeom): the workgroup reads its map entry
//      with one uniform load, then the descriptor through the constant address
//      space; the ragged last tile is masked by the segment's own chunk count,
//      output offsets are taken within the segment's own stripes.
#include <hip/hip_runtime.h>

#include "rs_sets_tile.hpp"
#include "rs_sized.hpp"

namespace uplink_ec {
namespace {

using namespace dev;

__global__ __launch_bounds__(256) void rs_sized_prep(const SizedStage *stage, SizedDesc *desc, uint64_t jt_base) {
    const SizedStage *st = stage + blockIdx.x;
    const int tid = threadIdx.x;
    copy_desc(&st->d, desc + blockIdx.x);
    if (tid == 0) {
        uint32_t *zc = st->d.zero_check;
        if (zc) *zc = 0u;
    }
    // the segment's tiles of its class's map: all this segment
    uint32_t *map = st->map;
    const int64_t ntiles = st->ntiles;
    for (int64_t i = tid; i < ntiles; i += blockDim.x) map[i] = blockIdx.x;
    write_leaves(st->coef, st->entries, st->d.tgt, jt_base);
}

// The map and the descriptors are read through the constant address space: the
// kernel never writes them, and uniform loads from there are scalar loads.
typedef const __attribute__((address_space(4))) SizedDesc ConstDesc;
typedef const __attribute__((address_space(4))) uint32_t ConstMap;

struct SizedGeom : StripeGeom<ConstDesc> {
    static constexpr bool kOwnTable = false;
    const SizedArgs &a;
    const int64_t tile;  // the workgroup's tile within its segment

    // ctile: the workgroup's tile of the class; its segment through the map
    __device__ __forceinline__ SizedGeom(const SizedArgs &a_, int64_t ctile)
        : StripeGeom<ConstDesc>{(ConstDesc *)(a_.desc +
                                              (uint32_t)__builtin_amdgcn_readfirstlane(((ConstMap *)a_.map)[ctile]))},
          a(a_), tile(ctile - d->tile0) {}
    __device__ __forceinline__ bool skip(int nin, int) const { return nin <= 0 || tile < 0; }
    // the tile's two chunks of 16 byte columns per lane, masked by the segment's own chunk count
    __device__ __forceinline__ void cols(int lane) { stripe_cols(tile * kTileChunks + lane, d->chunks, a.cps, a.ess, a.k); }
    __device__ __forceinline__ bool in_ok(const uint8_t *p, const uint8_t *share) const {
        return in_span(a, p, share, d->piece_len, 12);
    }
    __device__ __forceinline__ bool out_ok(const uint8_t *p, const uint8_t *) const {
        return in_span(a, p, out, d->spad, 13);
    }
};

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_matmul_sized(const SizedArgs a) {
    SizedGeom G(a, a.tile_base + blockIdx.x);
    share_tile<NW>(G);
}

}  // namespace

hipError_t launch_sized_prep(const SizedStage *stage, SizedDesc *desc, int nseg, uint64_t jt_base, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_sized_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base);
    return hipGetLastError();
}

hipError_t launch_matmul_sized(const SizedArgs &a, int nw, hipStream_t s) {
    return launch_share_tile(a, a.total_tiles, nw, s, rs_matmul_sized<2>, rs_matmul_sized<3>, rs_matmul_sized<4>);
}

}  // namespace uplink_ec
