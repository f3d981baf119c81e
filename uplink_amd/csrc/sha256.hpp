// SHA-256 piece hashing on the GPU (pb.PieceHashAlgorithm_SHA256,
// private/piecestore/hash.go:15-26): launch entry points used by the C-ABI.
// Host-only header, plain pointers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace uplink_ec {

// One lane of a list pass, in device memory: byte t of its piece at
// base + (t >> run_shift)*run_stride + (t & (run - 1)) when `fast`, at
// base + (t / run)*run_stride + t % run otherwise (a contiguous piece: run =
// 2^62, run_stride = 0; b3_list_geom.hpp run_of).  hash == nullptr: a padding lane.
struct ShaDesc {
    const uint8_t *base;
    uint64_t len;
    uint64_t run;
    int64_t run_stride;
    uint8_t *hash;  // where its 32 bytes go
    int32_t run_shift;
    uint32_t fast;  // sha_list_geom.hpp kFast: 16-byte loads
    uint64_t rsv[2];
};
static_assert(sizeof(ShaDesc) == 64, "staged as 16-byte words");

// One pass of a list: `stage_bytes` of host-written descriptors at h_stage are
// copied to d_stage by a kernel; then `launches` launches of `lanes` lanes (a
// multiple of 64), each advancing every unfinished piece by at most
// launch_blocks blocks, its eight state words kept in `state` in between.
struct ShaListPass {
    const void *h_stage;  // pinned, 16-byte aligned
    void *d_stage;
    size_t stage_bytes;  // a multiple of 16
    const ShaDesc *desc;  // in d_stage, one per lane
    uint32_t lanes;
    uint32_t *state;  // lanes * 8 words
    uint64_t launch_blocks, launches;
    // checked build: the declared range of the digest stores and the violation word
    uint8_t *hash_lo, *hash_hi;
    uint32_t *chk_flag;
};
hipError_t sha256_launch_list(const ShaListPass &p, hipStream_t stream);

// npieces pieces of piece_len bytes, byte t of piece j at
// base + j*piece_stride + (t / run)*run_stride + t % run (run = 0: contiguous).
// hashes: npieces*32 device bytes.  `state`: npieces*32 bytes of scratch when
// sha256_uniform_launches() > 1, else unused.
struct ShaView {
    const uint8_t *base;
    int64_t piece_stride;
    uint64_t piece_len;
    uint64_t run;
    int64_t run_stride;
    uint64_t npieces;
};
uint64_t sha256_uniform_launches(const ShaView &v, uint64_t launch_blocks);
hipError_t sha256_launch_uniform(const ShaView &v, uint8_t *hashes, uint32_t *state, uint64_t launch_blocks,
                                 hipStream_t stream);

}  // namespace uplink_ec
