// Segment repair (include/uplink_ec.h ec_repair_segments_sets): from the k
// basis shares of a segment, the pieces that were lost, piece layout in and
// out.  Reference: the repair / graceful-exit callers of ecclient.Client
// (private/ecclient/client.go:36-44), which today fetch k pieces, decode the
// segment and encode it again.
//
// Per call the host writes, per segment, a RepairStage into pinned memory: the
// descriptor (share and output pointers, row counts) and where its rows'
// coefficients sit, already in the order of the leaf table ([pass][input]
// [group][8], rows right-aligned per group, one byte each).  rs_repair_prep (one
// workgroup per segment) copies the descriptor to device memory and turns the
// coefficients into jump-table leaf addresses; rs_repair<NW> then computes one
// 2048-column tile per workgroup.  All of it is stream-ordered on the caller's
// stream.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_args.hpp"
#include "rs_rows.hpp"

namespace uplink_ec {

constexpr int kRepairMaxOut = 256;  // targets of one segment (n <= 256)

// One segment of a repair launch, in device memory.
struct RepairDesc {
    const uint8_t *in[kMaxOps];    // input shares: the k basis shares, then (check) the other shares; piece_len bytes each
    uint8_t *out[kRepairMaxOut];   // regenerated piece of row r < nstore, piece_len bytes
    uint64_t *tgt;                 // leaf addresses [pass][input][group][8] (rs_repair_prep)
    int32_t *status;               // check: this segment's status word (rows from nstore on are syndrome rows); else null
    int32_t nin, nout, nstore, nw;
};
static_assert(sizeof(RepairDesc) % 8 == 0, "copied as 8-byte words");

// What the host writes per segment (pinned memory, read once by rs_repair_prep).
struct RepairStage {
    RepairDesc d;
    const uint8_t *coef;  // pinned: the leaf table's coefficients, entries bytes (a multiple of 16)
    int64_t entries;
};

// Kernel arguments of rs_repair (one launch per wave-count class).
struct RepairArgs {
    const RepairDesc *desc;  // this launch's segments
    int64_t piece_len;       // nstripes * ess
    int64_t chunks_per_seg;  // piece_len / 16
    int64_t tiles_per_seg, total_tiles;
    uint32_t *chk_flag;      // checked build: first access outside a share / an output (site 10 or 11)
};

// ---- segments of different sizes in one call (ec_repair_segments_sized) ----
// The same with the geometry that RepairArgs carries for the whole launch read
// from the tile's segment instead, as the sized Rebuild does (rs_sized.hpp): a
// tile finds its segment through a map of the launch's class, one uint32 per
// tile, the position of its segment's descriptor in the pass.

// One segment of a sized repair pass, in device memory: RepairDesc plus the
// segment's own geometry (as SizedDesc carries it).
struct RepairSizedDesc {
    const uint8_t *in[kMaxOps];    // input shares: the k basis shares, then (check) the other shares; piece_len bytes each
    uint8_t *out[kRepairMaxOut];   // regenerated piece of row r < nstore, piece_len bytes
    uint64_t *tgt;                 // leaf addresses [pass][input][group][8] (rs_repair_sized_prep)
    int32_t *status;               // check: this segment's status word (rows from nstore on are syndrome rows); else null
    int32_t nin, nout, nstore, nw;
    int64_t chunks;                // 16-byte chunks of one piece: piece_len / 16 (fits 32 bits)
    int64_t piece_len;             // nstripes * ess
    int64_t tile0;                 // its first tile in its class's tile numbering
};
static_assert(sizeof(RepairSizedDesc) % 8 == 0, "copied as 8-byte words");

// What the host writes per segment (pinned memory, read once by rs_repair_sized_prep).
struct RepairSizedStage {
    RepairSizedDesc d;
    const uint8_t *coef;  // pinned: the leaf table's coefficients, entries bytes (a multiple of 16)
    int64_t entries;
    uint32_t *map;        // device: the segment's range of its class's map, ntiles entries
    int64_t ntiles;
};

// Kernel arguments of rs_repair_sized (one launch per wave-count class, or per
// part of one).
struct RepairSizedArgs {
    const RepairSizedDesc *desc;  // the pass's descriptors
    const uint32_t *map;          // the class's map: [tile] -> position of its segment's descriptor
    int64_t tile_base;            // the launch's first tile of the class
    int64_t total_tiles;          // the launch's tiles
    uint32_t *chk_flag;           // checked build: first access outside a share / an output (site 14 or 15)
};

// waves per workgroup for `rows` computed rows: as sets_waves up to 32 rows, 8
// waves above (up to 64 rows in one pass over the inputs)
int repair_waves(int rows);
// (one segment's coefficient staging and leaf table on nw waves: staged_entries bytes and words;
// a launch: at most share_max_tiles(nw) tiles -- rs_rows.hpp)
hipError_t launch_repair_prep(const RepairStage *stage, RepairDesc *desc, int nseg, uint64_t jt_base, hipStream_t s);
hipError_t launch_repair(const RepairArgs &a, int nw, hipStream_t s);
hipError_t launch_repair_sized_prep(const RepairSizedStage *stage, RepairSizedDesc *desc, int nseg, uint64_t jt_base,
                                    hipStream_t s);
// nw: 2, 3, 4 or 8 (repair_waves); at most share_max_tiles(nw) tiles
hipError_t launch_repair_sized(const RepairSizedArgs &a, int nw, hipStream_t s);
// byte path with the share check: the rows of `a` (coef, in_off, nin, nout as
// launch_matmul_bytes reads them) are compared with the bytes at out_off[r]
// instead of stored; any difference sets *a.zero_check to 1
hipError_t launch_repair_check_bytes(const RsArgs &a, hipStream_t s);

}  // namespace uplink_ec
