// Encode of a batch of segments that each have their own size
// (include/uplink_ec.h ec_encode_segments_sized): the uploads in flight at once
// are of as many sizes as there are objects (single.go:233-238 pads and encodes
// each segment from its own length; segmentupload/encode.go:39-75 reads the
// pieces of one segment), and one stream-ordered pass serves them all.
//
// The kernel is the compile-time-G encoder's body (rs_encoder.hpp) with the
// geometry it takes from the launch -- blocks, chunks and piece length per
// segment -- read from the block's segment descriptor instead
// (rs_encoder_sized.hpp).  The unit stays the encoder's: a block is 64 chunks of
// 16 B of every share row, all of one segment; a tile is block t and block
// t + ceil(B / 2) of the B blocks of the pass's segments concatenated, so its
// two blocks usually lie in different segments of different piece length.  A
// block finds its segment through a map: one uint32 per block, the position of
// its segment's descriptor in the pass.  Per pass the host writes, per segment,
// an EncSizedStage into pinned memory; rs_encode_sized_prep (one workgroup per
// segment) copies the descriptor to device memory, fills the segment's range of
// the map and, for a segment given by its data length, writes PadReader's
// padding behind the data; rs_encode_sized<K, N, ...> (rs_encode_aot.hip, one
// per library-built code) then encodes.  All of it is stream-ordered on the
// caller's stream.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_kernels.hpp"

namespace uplink_ec {

// One segment of a sized encode pass, in device memory.
struct EncSizedDesc {
    const uint8_t *in;   // the segment, stripe-major [stripe][k][ess]
    uint8_t *out;        // its pieces [n][piece_len] (parity only: [n-k][piece_len])
    int64_t chunks;      // 16-byte chunks of one share: nstripes * ess / 16 (fits 32 bits)
    int64_t piece_len;   // nstripes * ess
    int64_t block0;      // its first block among the pass's blocks
};
static_assert(sizeof(EncSizedDesc) == 40, "copied as 8-byte words");

// What the host writes per segment (pinned memory, read once by rs_encode_sized_prep).
struct EncSizedStage {
    EncSizedDesc d;
    int64_t nblocks;    // its blocks: entries [block0, block0 + nblocks) of the map
    uint64_t data_len;  // with pad > 0: the padding goes to in[data_len ..]
    uint32_t pad;       // PadReader's byte count p (0: the segment is already padded)
    uint32_t rsv;
};

// Kernel arguments of rs_encode_sized.
struct EncSizedArgs {
    const EncSizedDesc *desc;   // the pass's descriptors
    const uint32_t *map;        // [block] -> position of its segment's descriptor
    int64_t total_blocks;       // the pass's blocks
    uint32_t *queue;            // RsArgs::queue
    uint32_t *queue_host_done;  // RsArgs::queue_host_done
    uint32_t queue_seq;
    int32_t ess, cps;           // share size, ess / 16
    uint32_t *chk_flag;         // checked build: first access outside a segment's input / pieces (sites 21-23)
};

hipError_t launch_encode_sized_prep(const EncSizedStage *stage, EncSizedDesc *desc, uint32_t *map, int nseg,
                                    hipStream_t s);
// e: a library-built encoder (aot_encoder); grid 0: default_grid of the pass's tiles
hipError_t launch_encode_sized(const EncoderKernel &e, const EncSizedArgs &a, bool parity_only, int grid,
                               hipStream_t s);

}  // namespace uplink_ec
