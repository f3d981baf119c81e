// Encode of segments of different sizes (rs_encode_sized.hpp).
//
//  rs_encode_sized_prep: one workgroup per segment copies its descriptor from
//      the host's staging to device memory, fills the segment's range of the
//      block map with the segment's position and, for a segment given by its
//      data length, writes PadReader's padding behind the data (the bytes
//      ec_pad_segments writes: p times the byte p, the last 4 p big-endian).
//  rs_encode_sized<K, N, NC, NL, COPY>: rs_encoder_sized.hpp, instantiated per
//      library-built code in rs_encode_aot.hip; launched here.
#include <hip/hip_runtime.h>

#include "rs_encode_sized.hpp"

namespace uplink_ec {
namespace {

__global__ __launch_bounds__(256) void rs_encode_sized_prep(const EncSizedStage *stage, EncSizedDesc *desc,
                                                            uint32_t *map) {
    const EncSizedStage *st = stage + blockIdx.x;
    const int tid = threadIdx.x;
    {
        const uint64_t *src = (const uint64_t *)&st->d;
        uint64_t *dst = (uint64_t *)(desc + blockIdx.x);
        for (int i = tid; i < (int)(sizeof(EncSizedDesc) / 8); i += blockDim.x) dst[i] = src[i];
    }
    // the segment's blocks of the map: all this segment
    uint32_t *m = map + st->d.block0;
    const int64_t nblocks = st->nblocks;
    for (int64_t i = tid; i < nblocks; i += blockDim.x) m[i] = blockIdx.x;
    // the padding: at most a stripe and 3 bytes
    const uint32_t p = st->pad;
    if (p) {
        uint8_t *tail = const_cast<uint8_t *>(st->d.in) + st->data_len;
        for (uint32_t i = tid; i < p; i += blockDim.x) {
            uint8_t v = (uint8_t)p;
            if (i + 4 >= p) v = (uint8_t)(p >> (8 * (p - 1 - i)));  // last 4 bytes: big-endian p
            tail[i] = v;
        }
    }
}

}  // namespace

hipError_t launch_encode_sized_prep(const EncSizedStage *stage, EncSizedDesc *desc, uint32_t *map, int nseg,
                                    hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_encode_sized_prep, dim3(nseg), dim3(256), 0, s, stage, desc, map);
    return hipGetLastError();
}

hipError_t launch_encode_sized(const EncoderKernel &e, const EncSizedArgs &args, bool parity_only, int grid,
                               hipStream_t s) {
    const EncoderKernel::Variant &v = parity_only ? e.sized_parity : e.sized_full;
    if (!v.aot) return hipErrorInvalidDeviceFunction;  // (a run-time-compiled encoder has no sized form)
    if (args.total_blocks <= 0) return hipSuccess;
    if (grid <= 0) grid = default_grid((args.total_blocks + 1) / 2, v.wgs_per_cu);  // tiles = pairs of blocks
    EncSizedArgs a = args;
    void *params[] = {&a};
    return hipLaunchKernel(v.aot, dim3(grid), dim3(v.threads), params, 0, s);
}

}  // namespace uplink_ec
