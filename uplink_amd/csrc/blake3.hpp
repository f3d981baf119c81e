// BLAKE3-256 piece hashing on the GPU: launch entry
// points used by the C-ABI.  Host-only header, plain pointers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace uplink_ec {

// npieces byte strings of piece_len bytes each, in sets of pieces_per_set
// (0 = one set).  Byte t of string j lives at
//   base + (j / pieces_per_set)*set_stride + (j % pieces_per_set)*piece_stride
//        + (t / run)*run_stride + t % run
// (run = piece_len for contiguous pieces; run = ess, run_stride = k*ess for
// the data pieces of a stripe-major segment).
struct B3View {
    const uint8_t *base;
    int64_t piece_stride;
    uint64_t piece_len;
    uint64_t run;
    int64_t run_stride;
    uint64_t npieces;
    uint64_t pieces_per_set;
    int64_t set_stride;
    int32_t run_shift;  // set by b3_launch: log2(run) when run is a power of two, else -1
#ifdef UPLINK_EC_CHECKED
    // checked build, list kernels: every load is compared with the piece's own
    // extent and a violation's site recorded here (nullptr: the uniform launches, unchecked)
    uint32_t *chk_flag;
#endif
};

// ---- a list of pieces that each have their own length (ec_blake3_pieces_list,
// ec_hash_segments_sized; geometry in b3_list_geom.hpp) ----
// One piece of a pass, in device memory: byte t at base + (t >> run_shift)*run_stride
// + (t & (run - 1)) on the fast path, base + (t / run)*run_stride + t % run on the
// byte path (a contiguous piece: run = 2^62, run_stride = 0).
struct B3ListDesc {
    const uint8_t *base;
    uint64_t len;
    uint64_t run;
    int64_t run_stride;
    uint8_t *hash;     // where its 32 bytes go
    uint32_t wg0;      // its first workgroup in its launch (the fast or the byte pieces')
    uint32_t node0;    // its first node slot (pieces of >= 2 groups)
    uint32_t groups;   // its 256-chunk groups: 1 .. 256
    int32_t run_shift;
    uint64_t rsv;
};
static_assert(sizeof(B3ListDesc) == 64, "staged as 16-byte words");

// One pass: `stage_bytes` of host-written staging (descriptors, the two launches'
// workgroup -> piece maps, the parents list) at h_stage are copied to d_stage by a
// kernel, and desc / map_* / parents point into d_stage.  Then at most two chunk
// launches (fast and byte pieces) and one parents launch, stream-ordered.
struct B3ListPass {
    const void *h_stage;  // pinned, 16-byte aligned
    void *d_stage;
    size_t stage_bytes;   // a multiple of 16
    const B3ListDesc *desc;
    const uint32_t *map_fast, *map_byte, *parents;
    uint32_t wgs_fast, wgs_byte, nparents;
    uint32_t *nodes;      // node scratch, node_cap slots of 32 bytes
    uint32_t node_cap;
    // checked build: the declared range of the hash stores and the violation word
    uint8_t *hash_lo, *hash_hi;
    uint32_t *chk_flag;
};
hipError_t b3_launch_list(const B3ListPass &p, hipStream_t stream);

// Device bytes of scratch b3_launch needs for this view (0 when every piece
// fits one 256-chunk group).
size_t b3_workspace_bytes(const B3View &v);

// hashes: npieces*32 bytes on the device.  `ws` has b3_workspace_bytes(v).
hipError_t b3_launch(const B3View &v, uint8_t *hashes, void *ws, hipStream_t stream);
// Both views in one launch (equal piece_len): hashes of `first`'s pieces,
// then `second`'s.  ws: b3_workspace_bytes of a view with the summed npieces.
hipError_t b3_launch2(const B3View &first, const B3View &second, uint8_t *hashes, void *ws, hipStream_t stream);
// Streamed form (pieces of >= 2 chunks): the chaining values of BLAKE3 chunks
// [c0, c1) of every piece of both views into cvs [npieces][nchunks][8 words],
// as the bytes of those chunks become available; then b3_launch_fold turns the
// complete cvs into the hashes (cvs is overwritten; ws: b3_fold_ws_bytes).
hipError_t b3_launch_chunk_range(const B3View &first, const B3View &second, uint64_t c0, uint64_t c1, uint32_t *cvs,
                                 hipStream_t stream);
size_t b3_fold_ws_bytes(uint64_t npieces, uint64_t nchunks);
hipError_t b3_launch_fold(uint32_t *cvs, uint64_t npieces, uint64_t nchunks, uint8_t *hashes, void *ws,
                          hipStream_t stream);

}  // namespace uplink_ec
