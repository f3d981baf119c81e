// AES-256-GCM segment encryption on the GPU: host-side
// key preparation and launch entry points used by the C-ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace uplink_ec {

// Per-key device data: the AES-256 round keys and 4-bit GHASH tables of
// H^1..H^64 (H = AES_K(0^128)), all words big-endian as GCM defines them.
struct GcmSched {
    uint32_t rk[60];
    uint32_t pad_[4];
    uint32_t htab[64][16][4];  // htab[p][nibble] = nibble * H^(p+1) (Shoup's 4-bit table)
    uint32_t h64_8[256][4];    // byte * H^64 (the 8-bit table of the Horner multiplier)
};

// Fills `out` with the schedule of a 32-byte key (host memory).
void gcm_prepare(const uint8_t key[32], GcmSched *out);

// One batch: nseg segments of nblocks GCM blocks each.  Block b of segment g
// is read from in + g*in_seg_stride + b*in_blk_stride (in_block plaintext
// bytes to seal, or in_block ciphertext bytes + 16-byte tag to open) and
// written to out + g*out_seg_stride + b*out_blk_stride (ciphertext || tag, or
// plaintext).  Its nonce is nonces[12*g..] + b (little-endian increment of
// the 12 bytes).  status[g] (open only, initialised by the launcher) ends as
// the first block of segment g whose tag did not verify, or -1.
struct GcmBatch {
    const uint8_t *in;
    uint8_t *out;
    int64_t in_seg_stride, out_seg_stride;
    int64_t in_blk_stride, out_blk_stride;
    const GcmSched *sched;  // [nseg] device
    const uint8_t *nonces;  // [nseg][12] device
    int32_t *status;        // [nseg] device (open)
    uint32_t nseg, nblocks, in_block;
};

hipError_t gcm_launch(const GcmBatch &b, bool open, hipStream_t stream);

// The workgroups the uniform launch spreads over a batch (256 * UPLINK_GCM_GRID_PER_CU).
uint32_t gcm_target_grid();

// status[0..nseg) to "nothing failed yet" before the first launch of an open
// (fini false), and the words still so to -1 after the last (fini true).
hipError_t gcm_status_launch(int32_t *status, uint32_t nseg, bool fini, hipStream_t stream);

// ---- segments of different sizes in one launch (include/uplink_ec.h
// ec_gcm_seal_segments_sized / ec_gcm_open_segments_sized) ----
//
// A pass is a list of segments, each of its own number of dense GCM blocks, with
// its own workgroups (gcm_sized_geom.hpp).  A workgroup finds its segment through
// a map: one uint32 per workgroup, the position of its segment's descriptor in
// the pass.  Per pass the host writes a GcmSizedStage per segment into pinned
// memory; gcm_sized_prep (one workgroup per segment) copies the descriptor to
// device memory, fills the segment's workgroups' entries of the map and, for a
// segment given by its data length, writes PadReader's padding behind the data;
// gcm_blocks_sized then runs the uniform kernel's block body over each segment.

// One segment of a pass, in device memory.
struct GcmSizedDesc {
    const uint8_t *in;   // nblocks dense blocks: in_block bytes each to seal, in_block + 16 to open
    uint8_t *out;        // nblocks dense blocks: in_block + 16 bytes each sealed, in_block opened
    uint32_t nblocks;
    uint32_t wg0, wgs;   // its first workgroup in the pass's grid and how many it has
    uint32_t seg;        // its index in the call: key, nonce and status word
};
static_assert(sizeof(GcmSizedDesc) == 32, "copied as 8-byte words");

// What the host writes per segment (pinned memory, read once by gcm_sized_prep).
struct GcmSizedStage {
    GcmSizedDesc d;
    uint64_t data_len;  // with pad > 0: the padding goes to in[data_len ..]
    uint32_t pad;       // PadReader's byte count p (0: the segment is already padded)
    uint32_t rsv;
};

// Kernel arguments of gcm_blocks_sized.
struct GcmSizedArgs {
    const GcmSizedDesc *desc;  // the pass's descriptors
    const uint32_t *map;       // [workgroup] -> position of its segment's descriptor
    const GcmSched *sched;     // [nseg] of the call
    const uint8_t *nonces;     // [nseg][12] of the call
    int32_t *status;           // [nseg] of the call (open)
    uint32_t *chk_flag;        // checked build: first access outside a segment's extents (sites 41-44)
    uint32_t in_block, nseg;
};

// One pass: the prep launch, then the cipher, on `stream`.
struct GcmSizedPass {
    const GcmSizedStage *stage;  // [n] pinned, device-visible
    GcmSizedDesc *desc;          // [n] device
    uint32_t *map;               // [wgs] device
    uint32_t n, wgs;
    const GcmSched *sched;
    const uint8_t *nonces;
    int32_t *status;
    uint32_t nseg, in_block;
    uint32_t *chk_flag;
};
hipError_t gcm_launch_sized(const GcmSizedPass &p, bool open, hipStream_t stream);

// ---- ranges of segments opened in one launch (include/uplink_ec.h
// ec_gcm_open_ranges_sized; range_geom.hpp) ----
//
// A segment of a pass is a run of nblocks covered blocks, first_block .. of the
// download's segment, of which the plaintext bytes [head, head + length) are
// wanted: relative block r is opened under nonce + (first_block + r), every
// covered block is read and authenticated whole, and only the wanted bytes are
// stored, dense, at out.  The pass, its map and its workgroups are the sized
// cipher's (gcm_sized_geom.hpp).

constexpr uint32_t kGcmRangedBytewise = 1;  // GcmRangedDesc::flags: a source or output slot is not 16-byte aligned

// One segment of a pass: written by the host to pinned memory, copied to device
// memory by gcm_ranged_prep.
struct GcmRangedDesc {
    const uint8_t *in;   // nblocks dense blocks of in_block + 16 bytes, at any alignment
    uint8_t *out;        // length bytes, at any alignment
    uint64_t length;     // plaintext bytes wanted
    uint32_t head;       // the first of them is byte `head` of the first covered block (head < in_block)
    uint32_t nblocks, first_block;
    uint32_t wg0, wgs;   // its first workgroup in the pass's grid and how many it has
    uint32_t seg;        // its index in the call: key, nonce and status word
    uint32_t flags, rsv;
};
static_assert(sizeof(GcmRangedDesc) == 56, "copied as 8-byte words");

// Kernel arguments of gcm_open_ranged.
struct GcmRangedArgs {
    const GcmRangedDesc *desc;  // the pass's descriptors
    const uint32_t *map;        // [workgroup] -> position of its segment's descriptor
    const GcmSched *sched;      // [nseg] of the call
    const uint8_t *nonces;      // [nseg][12] of the call: each segment's starting nonce
    int32_t *status;            // [nseg] of the call
    uint32_t *chk_flag;         // checked build: first access outside a segment's extents (sites 41-43)
    uint32_t in_block, nseg;
};

// One pass: the prep launch, then the cipher, on `stream`.
struct GcmRangedPass {
    const GcmRangedDesc *stage;  // [n] pinned, device-visible
    GcmRangedDesc *desc;         // [n] device
    uint32_t *map;               // [wgs] device
    uint32_t n, wgs;
    const GcmSched *sched;
    const uint8_t *nonces;
    int32_t *status;
    uint32_t nseg, in_block;
    uint32_t *chk_flag;
    bool mixed;                  // a segment of the pass has kGcmRangedBytewise set
};
hipError_t gcm_launch_ranged(const GcmRangedPass &p, hipStream_t stream);

// ---- one-shot messages, a raw key each (include/uplink_ec.h
// ec_gcm_seal_messages / ec_gcm_open_messages; gcm_msg_geom.hpp,
// gcm_msg_device.hpp) ----
//
// A message is one GCM seal or open of len bytes (0 .. 1 << 24) under its own
// 32-byte key and 12-byte nonce: J0 = nonce || 1, counters from 2, no AAD, the
// sealed form ciphertext || tag.  One wave takes a message and derives everything
// from the key bytes itself -- round keys, H, the powers of H its layout needs --
// so there is no GcmSched and no host-side key preparation.  Meant for many short
// messages (inline segments up to 4 KiB, 32-byte content keys); a long message is
// still spread over its wave's 64 lanes, but one wave is all it gets.

// One message of a pass: written by the host to pinned memory, copied to device
// memory by gcm_msg_prep.
struct GcmMsgDesc {
    const uint8_t *in;  // len bytes to seal, len + 16 to open; any alignment
    uint8_t *out;       // len + 16 bytes sealed, len opened; any alignment
    uint32_t len;
    uint32_t msg;       // its index in the call: key, nonce and status word
};
static_assert(sizeof(GcmMsgDesc) == 24, "copied as 8-byte words");

// Kernel arguments of gcm_messages.
struct GcmMsgArgs {
    const GcmMsgDesc *desc;  // the pass's descriptors
    const uint8_t *keys;     // [nmsg][32] of the call, raw key bytes
    const uint8_t *nonces;   // [nmsg][12] of the call
    int32_t *status;         // [nmsg] of the call (open): 0, or 1 when the tag did not verify
    uint32_t *chk_flag;      // checked build: first access outside a message's extents (sites 51-53)
    uint32_t n, nmsg;        // messages of the pass, of the call
};

// One pass: the prep launch, then the cipher, on `stream`.
struct GcmMsgPass {
    const GcmMsgDesc *stage;  // [n] pinned, device-visible
    GcmMsgDesc *desc;         // [n] device
    uint32_t n;
    const uint8_t *keys, *nonces;
    int32_t *status;
    uint32_t nmsg;
    uint32_t *chk_flag;
};
hipError_t gcm_launch_messages(const GcmMsgPass &p, bool open, hipStream_t stream);

// AES-256 of one block on the host (key setup and tests)
void aes256_encrypt_block(const uint32_t rk[60], const uint8_t in[16], uint8_t out[16]);

}  // namespace uplink_ec
