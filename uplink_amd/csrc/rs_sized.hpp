// Rebuild / Decode of a batch of segments that each come with their own share
// set and their own size (include/uplink_ec.h ec_rebuild_segments_sized,
// ec_decode_segments_sized): the downloads in flight at once are of as many
// sizes as there are objects (private/ecclient/client.go:302-303 sizes each
// from its own `size`), and one stream-ordered pass serves them all.
//
// The tile body is the one rs_matmul_sets runs (rs_sets_tile.hpp) with the
// geometry that kernel takes from the launch -- stripes, chunks and tiles per
// segment -- read from the tile's segment descriptor instead.  A tile finds its segment through a map
// of the launch's class: one uint32 per tile, the position of its segment's
// descriptor in the pass.  Per pass the host writes, per segment, a SizedStage
// into pinned memory (the descriptor, the rows' coefficients in leaf-table
// order, solved on the host); rs_sized_prep (one workgroup per segment) copies
// the descriptor to device memory, turns the coefficients into jump-table leaf
// addresses, fills the segment's range of the map and zeroes its syndrome
// counter; rs_matmul_sized<NW> then computes one 2048-column tile per
// workgroup.  All of it is stream-ordered on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_args.hpp"
#include "rs_rows.hpp"

namespace uplink_ec {

// One segment of a sized pass, in device memory: SetDesc (rs_sets.hpp) plus
// the segment's own geometry.
struct SizedDesc {
    const uint8_t *in[kMaxOps];  // the segment's input shares (the k basis shares first), piece_len bytes each
    uint8_t *out;                // the segment, stripe-major [stripe][k][ess], spad bytes
    uint64_t *tgt;               // leaf addresses [pass][input][group][8] (rs_sized_prep)
    uint32_t *zero_check;        // Decode: this segment's syndrome counter (rows from nstore on); null: Rebuild
    int32_t nin, nout, nstore, pad;
    int64_t chunks;              // 16-byte chunks of one share: nstripes * ess / 16 (fits 32 bits)
    int64_t piece_len;           // nstripes * ess
    int64_t spad;                // piece_len * k
    int64_t tile0;               // its first tile in its class's tile numbering
    int32_t copy_off[kMaxOps];   // byte offset within a stripe of the output a basis data share is copied to, -1 none
    int32_t out_off[kMaxOps];    // byte offset within a stripe of computed row r (rows < nstore)
};
static_assert(sizeof(SizedDesc) % 8 == 0, "copied as 8-byte words");

// What the host writes per segment (pinned memory, read once by rs_sized_prep).
struct SizedStage {
    SizedDesc d;
    const uint8_t *coef;  // pinned: the leaf table's coefficients, entries bytes (a multiple of 16)
    int64_t entries;
    uint32_t *map;        // device: the segment's range of its class's map, ntiles entries
    int64_t ntiles;
};

// Kernel arguments of rs_matmul_sized (one launch per wave-count class, or per
// part of one).
struct SizedArgs {
    const SizedDesc *desc;  // the pass's descriptors
    const uint32_t *map;    // the class's map: [tile] -> position of its segment's descriptor
    int64_t tile_base;      // the launch's first tile of the class
    int64_t total_tiles;    // the launch's tiles
    int32_t ess, cps, k, pad;
    uint32_t *chk_flag;     // checked build: first access outside a share / an output (site 12 or 13)
};

// (one segment's coefficient staging and leaf table on nw waves: staged_entries bytes and words, rs_rows.hpp)
hipError_t launch_sized_prep(const SizedStage *stage, SizedDesc *desc, int nseg, uint64_t jt_base, hipStream_t s);
// nw: 2, 3 or 4 (sets_waves); at most share_max_tiles(nw) tiles
hipError_t launch_matmul_sized(const SizedArgs &a, int nw, hipStream_t s);

}  // namespace uplink_ec
