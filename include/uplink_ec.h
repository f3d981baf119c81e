/*
 * uplink_ec.h — C ABI of the MI355X erasure-coding engine that replaces the
 * Reed-Solomon stripe loop of storj/uplink's private/eestream (+ the piece
 * fan-out of private/ecclient).  Plain pointers and sizes only; every compute
 * entry point runs on the GPU (HIP, gfx950).  There is no CPU fallback: if no
 * GPU is usable, ec_create returns EC_ERR_DEVICE.
 *
 * Reference interface each export replaces (storj/uplink @ /root/reference):
 *
 *   ec_create / ec_destroy   eestream.NewFEC + eestream.NewRSScheme
 *                            private/eestream/fec.go:15-17, rs.go:17-19
 *                            (called from encode.go:69-87)
 *   ec_required/total/share_size/stripe_size
 *                            ErasureScheme.RequiredCount/TotalCount/
 *                            ErasureShareSize/StripeSize   rs.go:47-61
 *   ec_encode_single         ErasureScheme.EncodeSingle    scheme.go:18, rs.go:21-23
 *                            (caller segmentupload/encode.go:58, eestream/encode.go:187)
 *   ec_encode                ErasureScheme.Encode          scheme.go:15, rs.go:25-30
 *   ec_rebuild               ErasureScheme.Rebuild         scheme.go:26, rs.go:40-45
 *                            (caller stripe.go:410-412)
 *   ec_decode                ErasureScheme.Decode          scheme.go:22, rs.go:32-38
 *                            (caller stripe.go:407-408; layout unsafe_rs.go:38-46)
 *   ec_encode_segments       batch form of EncodeSingle over every (piece, stripe)
 *                            of whole segments: segmentupload/encode.go:39-75 driven
 *                            by single.go:228-238 (pieceReader.PieceReader)
 *   ec_rebuild_segments      batch form of the per-stripe Rebuild loop of
 *                            StripeReader.ReadStripes  stripe.go:382-428
 *   ec_*_segments_sets       the same for many segments with a share set each:
 *                            one StripeReader per download, ecclient/client.go:273-308
 *   ec_*_segments_sized      the same with a stripe count per segment: GetWithOptions sizes
 *                            every download from its own size (client.go:302-303), so the
 *                            downloads in flight at once differ in size
 *   ec_repair_segments_sets  segment repair: the lost pieces regenerated from any k, a
 *                            share set per segment -- what the repair and graceful-exit
 *                            callers of ecclient.Client do with Get + PutSingleResult /
 *                            PutPiece (ecclient/client.go:36-44,77-101), without the
 *                            decoded segment in between
 *   ec_repair_segments_sized the same with a stripe count per segment: a repair queue
 *                            holds segments of as many sizes as there are objects
 *   ec_*_segments_host       the same batches from/to host memory (PCIe pipeline)
 *   ec_*blake3* / ec_hash_segments / ec_encode_segments_host_hashed
 *                            BLAKE3 piece hash of the upload (piecestore/upload.go:
 *                            133,155,270; hash.go:20-26), SURVEY §8f row 4
 *   ec_blake3_pieces_list / ec_hash_segments_sized
 *                            the same with a length per piece: the hashes of a batch of
 *                            uploads of different sizes in one pass
 *   ec_sha256_*              the SHA-256 piece hash (pb.PieceHashAlgorithm_SHA256,
 *                            hash.go:15-26): a list, a sized batch, pieces of one length
 *   ec_gcm_*                 AES-256-GCM segment encryption: splitter/splitter.go:156,170
 *                            (upload), streams/store.go:347-382 (download), SURVEY §8f row 4
 *   ec_gcm_seal_segments_sized / ec_gcm_open_segments_sized
 *                            the same with a block count, key and nonce per segment: the
 *                            cipher of a batch of different sizes in one pass
 *   ec_gcm_open_ranges_sized the open of a byte range of each segment of a batch: ranged
 *                            downloads (store.go:347-382 Range, eestream/decode.go:199-227)
 *   ec_strerror/ec_format_error  error texts of infectious / eestream
 *
 * Error codes map to the errors eestream's callers test:
 *   EC_ERR_NUM_NEGATIVE  "num must be non-negative"   (segmentupload/encode_test.go:53)
 *   EC_ERR_NUM_RANGE     "num must be less than %d"   (segmentupload/encode_test.go:63)
 *   EC_ERR_NOT_ENOUGH_SHARES  infectious.NotEnoughShares (stripe.go:446-449)
 *   EC_ERR_TOO_MANY_ERRORS    infectious.TooManyErrors   (stripe.go:446-449)
 *
 * Threading: an ec_ctx is immutable after ec_create except for internal
 * caches guarded by a mutex; every export is reentrant (uplink calls
 * EncodeSingle from up to 300 goroutines, private/testuplink/uplink.go:83).
 * No pointer passed in is retained after a call returns (cgo rules);
 * the *_segments calls are asynchronous on `stream` and the caller keeps the
 * device buffers alive until the stream is synchronised.
 */
#ifndef UPLINK_EC_H
#define UPLINK_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EC_OK 0
#define EC_ERR_PARAMS (-1)            /* "requires 1 <= k <= n <= 256" */
#define EC_ERR_NUM_NEGATIVE (-2)      /* "num must be non-negative" */
#define EC_ERR_NUM_RANGE (-3)         /* "num must be less than %d" (n) */
#define EC_ERR_INPUT_LENGTH (-4)      /* "input length must be a multiple of %d" (k) */
#define EC_ERR_OUTPUT_LENGTH (-5)     /* "output length must be %d" */
#define EC_ERR_NOT_ENOUGH_SHARES (-6) /* infectious.NotEnoughShares */
#define EC_ERR_TOO_MANY_ERRORS (-7)   /* infectious.TooManyErrors */
#define EC_ERR_INVALID_SHARE (-8)     /* "invalid share id: %d" */
#define EC_ERR_SINGULAR (-9)          /* decode matrix not invertible */
#define EC_ERR_INVALID_ARG (-10)      /* null pointer / bad size / layout */
#define EC_ERR_DEVICE (-11)           /* HIP runtime error or no GPU */
#define EC_ERR_UNSUPPORTED (-12)      /* outside the engine's limits */
#define EC_ERR_SHARE_SIZE (-13)       /* shares of different lengths */
#define EC_ERR_AUTH (-14)             /* "cipher: message authentication failed" (a GCM tag did not verify) */

/* flags for ec_encode_segments */
#define EC_FLAG_PARITY_ONLY 0x1 /* write only the n-k parity pieces */
#define EC_FLAG_HASH_PIECES 0x2 /* ec_upload_begin: also the BLAKE3 of every piece (ec_upload_hashes) */
#define EC_FLAG_CHECK_SHARES 0x4 /* ec_repair_segments_sets: compare every share beyond the basis with the basis */

typedef struct ec_ctx ec_ctx;
typedef void *ec_stream; /* hipStream_t; NULL = the default stream */

int ec_create(int k, int n, int erasure_share_size, ec_ctx **out);
/* Every streamed upload (ec_upload_begin) of the context must have ended
 * (ec_upload_end) before ec_destroy; launches still queued on callers' streams
 * are waited for. */
void ec_destroy(ec_ctx *ctx);

int ec_required(const ec_ctx *ctx);
int ec_total(const ec_ctx *ctx);
int ec_share_size(const ec_ctx *ctx);
int ec_stripe_size(const ec_ctx *ctx);
/* copies the n x k generator matrix (row-major) into out (n*k bytes) */
int ec_generator(const ec_ctx *ctx, uint8_t *out);

const char *ec_strerror(int code);
/* message with the %d filled from ctx (n for NUM_RANGE, k for INPUT_LENGTH,
 * `arg` for OUTPUT_LENGTH / INVALID_SHARE); returns the message length */
int ec_format_error(const ec_ctx *ctx, int code, long long arg, char *buf, size_t len);

/* ---- ErasureScheme surface: host buffers, synchronous, GPU-computed ---- */

/* out (len(in)/k bytes) = erasure share `num` of the stripe `in` */
int ec_encode_single(const ec_ctx *ctx, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, int num);
/* all n shares of `in`: share i written to out + i*(in_len/k) */
int ec_encode(const ec_ctx *ctx, const uint8_t *in, size_t in_len, uint8_t *out);
/* Rebuild: `nums` (nshares entries) is sorted in place together with
 * `shares`, exactly as infectious sorts its []Share; the k data shares are
 * written to out + i*share_len. */
int ec_rebuild(const ec_ctx *ctx, int nshares, int *nums, const uint8_t **shares, size_t share_len, uint8_t *out);
/* Decode: Correct (Berlekamp-Welch when nshares > k) + Rebuild; `shares`
 * are corrected in place like infectious' share.Data.  out = k*share_len. */
int ec_decode(const ec_ctx *ctx, int nshares, int *nums, uint8_t **shares, size_t share_len, uint8_t *out);

/* ---- batched, device-resident (HIP device pointers), async on stream ---- */

/* segs: nseg padded segments, each nstripes*k*ess bytes, stripe-major
 *       [stripe][k][ess] (the PadReader output of single.go:234-236).
 * pieces: [nseg][n][nstripes*ess]  (or [nseg][n-k][...] with
 *       EC_FLAG_PARITY_ONLY).  Piece i of a segment = the concatenation of
 *       EncodeSingle(stripe, num=i) over its stripes. */
int ec_encode_segments(const ec_ctx *ctx, const uint8_t *segs, size_t nseg, size_t nstripes, uint8_t *pieces,
                       int flags, ec_stream stream);
/* ---- a size per segment (the upload path as uplink runs it) ----
 * The uploads in flight at once are of as many sizes as there are objects: the
 * last segment of every object has its own size, a small object is one short
 * segment (single.go:233-238 pads and encodes each segment from its own length;
 * segmentupload/encode.go:39-75 reads the n pieces of that one segment).  This
 * is ec_encode_segments with a stripe count per segment, in one stream-ordered
 * pass: segs[g] is a device pointer to segment g, nstripes[g]*k*ess bytes,
 * stripe-major as above; pieces[g] a device pointer to its [n][nstripes[g]*ess]
 * (or [n-k][...] with EC_FLAG_PARITY_ONLY), the layout ec_encode_segments
 * writes for one segment.
 * data_len == NULL: the segments are already padded and are only read.
 * data_len != NULL: segment g holds data_len[g] bytes, and the call writes
 * PadReader's padding behind them, in stream order before the encode: the
 * bytes ec_pad_segments(segs[g], 1, 0, data_len[g], k*ess, stream) writes.  It
 * requires nstripes[g]*k*ess == data_len[g] + p, p = 4 + (k*ess -
 * (data_len[g] + 4) % (k*ess)) % (k*ess); otherwise EC_ERR_INVALID_ARG.
 * Every segment is validated before anything is queued: on an argument error
 * nothing is written (a NULL segs[g] or pieces[g] with nstripes[g] > 0:
 * EC_ERR_INVALID_ARG; a segment whose nstripes[g]*ess/16 does not fit 32 bits:
 * EC_ERR_UNSUPPORTED).  nstripes[g] == 0 skips segment g: nothing of it is
 * looked at, and its pointers may be NULL.  Codes with a library-built
 * compile-time encoder (ec_encode_kernel_name "special", not "special-jit")
 * go through that encoder's sized form, each 1-KiB column block finding its
 * segment through a per-pass map; a segment of another code, with a share size
 * that is no multiple of 16 or with a pointer that is not 16-byte aligned goes
 * on its own through ec_pad_segments and ec_encode_segments' path with its own
 * stripe count; same results.  The call never starts a run-time compile.  A
 * batch of thousands of segments goes in passes of bounded staging.  Async on
 * stream, no host synchronisation once the staging pool is warm.  Not under
 * stream capture (EC_ERR_UNSUPPORTED).  Up to k = 128. */
int ec_encode_segments_sized(const ec_ctx *ctx, size_t nseg, uint8_t *const *segs, const size_t *nstripes,
                             const size_t *data_len /* may be NULL */, uint8_t *const *pieces, int flags,
                             ec_stream stream);
/* Rebuild whole segments from nshares >= k pieces (each nstripes*ess bytes,
 * device pointers in `pieces`, piece numbers in `nums`, any order).  The
 * share choice follows infectious Rebuild; out = nstripes*k*ess bytes,
 * stripe-major.  nseg segments may be batched with strides (in bytes,
 * 0 when nseg == 1). */
int ec_rebuild_segments(const ec_ctx *ctx, int nshares, const int *nums, const uint8_t *const *pieces,
                        size_t nstripes, uint8_t *out, ec_stream stream);
int ec_rebuild_segments_batched(const ec_ctx *ctx, int nshares, const int *nums, const uint8_t *const *pieces,
                                size_t nstripes, size_t nseg, long long piece_seg_stride, long long out_seg_stride,
                                uint8_t *out, ec_stream stream);
/* Decode whole segments with error detection: FEC.Decode (Correct +
 * Rebuild) on every stripe of the pieces at once -- what StripeReader runs
 * per stripe when error detection is on (private/eestream/stripe.go:407-408
 * -> rsScheme.Decode, rs.go:32-38).  Same arguments as ec_rebuild_segments;
 * with nshares > k every column is checked against the code (syndrome rows
 * computed and tested for zero inside the kernel, nothing stored) and, where
 * a column is not a codeword, corrected by Berlekamp-Welch.  Corrected
 * shares are written back into the caller's pieces, as infectious corrects
 * share.Data in place.  The check and the rebuild are one pass over the shares
 * (the rebuilt rows stored, the syndrome rows tested in the same kernel); a
 * segment with errors is then corrected and rebuilt again on its own.  Returns
 * when done (the check's outcome is read back), also when nshares == k:
 * EC_ERR_TOO_MANY_ERRORS / EC_ERR_NOT_ENOUGH_SHARES as Decode returns them.
 * Every share given is checked and corrected, as infectious' Correct uses
 * them all: of more than 128 (n > 128), the first 128 in number order go
 * through the one-pass check and the syndromes of the rest are checked in
 * further launches of up to 128 - k at a time. */
int ec_decode_segments(const ec_ctx *ctx, int nshares, const int *nums, uint8_t *const *pieces, size_t nstripes,
                       uint8_t *out, ec_stream stream);
/* The same over nseg segments in one check and one rebuild launch (strides as
 * ec_rebuild_segments_batched); a segment with errors is corrected on its own. */
int ec_decode_segments_batched(const ec_ctx *ctx, int nshares, const int *nums, uint8_t *const *pieces,
                               size_t nstripes, size_t nseg, long long piece_seg_stride, long long out_seg_stride,
                               uint8_t *out, ec_stream stream);

/* ---- a share set per segment (the download path as uplink runs it) ----
 * Every segment a download fetches is decoded from whichever k (or more)
 * pieces arrived first (StripeReader, private/eestream/stripe.go:314-354,
 * via ecclient GetWithOptions, private/ecclient/client.go:273-308, one per
 * segment, several at once under prefetch, private/storage/streams/
 * store.go:240-253,385-403): share sets are almost never repeated.  These
 * calls take nseg segments, each with its own set, in one pass: segment g's
 * shares are entries [off_g, off_g + nshares[g]) of nums / pieces (off_g the
 * sum of the nshares before it; device pointers, nstripes*ess bytes each, any
 * order), its output outs[g] (nstripes*k*ess bytes, stripe-major).  The share
 * choice is infectious Rebuild's per segment.  The decode rows of every
 * segment are solved on the GPU in stream order; the host only chooses the
 * shares (no synchronisation, no plan, no code generation on the call path).
 * A Rebuild of one segment (up to 64 shares) is one launch whose decode rows
 * the host solves and passes in the launch's arguments.
 *
 * ec_rebuild_segments_sets: Rebuild (stripe.go:410-412); async on stream. */
int ec_rebuild_segments_sets(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                             const uint8_t *const *pieces, size_t nstripes, uint8_t *const *outs, ec_stream stream);
/* Decode with error detection (stripe.go:407-408 -> rs.go:32-38) over the
 * same layout: one pass reads every share of every segment, stores the rebuilt
 * data and checks each segment's syndromes; a segment with errors is then
 * corrected in its pieces and rebuilt as ec_decode_segments does.  Returns
 * when done.  Segments of more than 128 shares go through ec_decode_segments. */
int ec_decode_segments_sets(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                            uint8_t *const *pieces, size_t nstripes, uint8_t *const *outs, ec_stream stream);
/* ---- a share set and a size per segment ----
 * The downloads in flight at once are of as many sizes as there are objects:
 * the last segment of every object has its own size, small objects are one
 * short segment each (GetWithOptions sizes every download from its own size,
 * client.go:302-303).  These calls are the share-set calls above with a stripe
 * count per segment, in one stream-ordered pass: each 2048-column tile finds
 * its segment through a per-launch map, and the segment's descriptor carries
 * its own geometry.  The decode rows are solved on the host in closed form (a
 * few microseconds per segment) and staged in event-recycled blocks; a batch of
 * thousands of segments goes in passes of bounded staging.  Every segment is
 * validated before anything is queued: on an argument error nothing is
 * written (too few shares, an invalid share number, a NULL pointer, a repeated
 * chosen share: EC_ERR_SINGULAR, a segment whose nstripes[g]*ess/16 does not
 * fit 32 bits: EC_ERR_UNSUPPORTED).  nstripes[g] == 0 skips segment g: nothing
 * of it is read or written and outs[g] may be NULL.  Segments whose share size
 * is no multiple of 16, or with a pointer that is not 16-byte aligned, go one
 * by one through ec_rebuild_segments / ec_decode_segments' path with their own
 * stripe count; same results.  Up to k = 128.  Not under stream capture
 * (EC_ERR_UNSUPPORTED).
 *
 * ec_rebuild_segments_sets with a stripe count per segment: segment g has
 * nstripes[g] stripes, its shares are nstripes[g]*ess bytes each, its output
 * nstripes[g]*k*ess bytes.  Async on stream. */
int ec_rebuild_segments_sized(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                              const uint8_t *const *pieces, const size_t *nstripes, uint8_t *const *outs,
                              ec_stream stream);
/* ec_decode_segments_sets likewise (up to 128 shares per segment in the pass;
 * segments with more go through ec_decode_segments on their own).  seg_rc
 * (host, nseg ints, may be NULL): segment g's own outcome (EC_OK,
 * EC_ERR_TOO_MANY_ERRORS, ...).  A failing segment does not stop the others:
 * every flagged segment is corrected in its pieces and rebuilt as
 * ec_decode_segments does, and the outputs of segments that succeeded are
 * complete.  EC_ERR_NOT_ENOUGH_SHARES is only ever the call's argument error
 * (a segment with fewer than k shares, nothing written): a segment in which an
 * error is detected but whose surplus is too small to correct any (fewer than
 * k + 2 shares, where infectious' Decode says NotEnoughShares) has
 * EC_ERR_TOO_MANY_ERRORS as its outcome.  Returns the first non-OK outcome in
 * segment order; returns when done. */
int ec_decode_segments_sized(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                             uint8_t *const *pieces, const size_t *nstripes, uint8_t *const *outs, int *seg_rc,
                             ec_stream stream);
/* Segment repair: regenerate lost pieces of nseg segments, each from its own
 * share set, without decoding the segment.  Shares are given exactly as for
 * ec_rebuild_segments_sets (flattened per segment, any order, device pointers
 * of nstripes*ess bytes each).  Segment g's targets are entries [toff_g,
 * toff_g + ntargets[g]) of `targets` (piece numbers, any order) and of `outs`
 * (device pointers of nstripes*ess bytes each, piece layout: what
 * ec_encode_segments writes for that piece); toff_g is the sum of the ntargets
 * before it.  A target must not be among the segment's shares.  The basis is
 * the k shares infectious Rebuild chooses, so a repair and a rebuild of one
 * share set trust the same shares; piece t is their Lagrange interpolation at
 * t's point, one GF(2^8) matrix per segment, solved on the host in closed form.
 * Async on stream, no host synchronisation, no caller memory retained.  Every
 * segment is validated before anything is queued: on an error nothing is
 * written.  ntargets[g] == 0 skips segment g.  Up to k = 128.
 *
 * Without EC_FLAG_CHECK_SHARES, shares beyond the basis are ignored and
 * dev_status may be NULL.  With it (at most 128 shares per segment), dev_status
 * (nseg device int32) is required: every non-basis share is predicted from the
 * basis in the same pass and compared (syndrome rows, nothing stored), and
 * dev_status[g] becomes 0 when all agreed, 1 when any byte differed -- the
 * segment's regenerated pieces must then not be used.  The status words are
 * zeroed in stream order by the call.  Correction is not part of this call:
 * for a flagged segment the caller runs ec_decode_segments on that segment's
 * pieces (it corrects them in place, or reports EC_ERR_TOO_MANY_ERRORS) and
 * repairs again.
 *
 * Segments whose share size is no multiple of 16, or with a pointer that is
 * not 16-byte aligned, go one by one through the byte kernel (their matrix is
 * uploaded as a cached plan on the context's own setup stream); same results. */
int ec_repair_segments_sets(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                            const uint8_t *const *pieces, const int *ntargets, const int *targets,
                            uint8_t *const *outs, size_t nstripes, int flags, int32_t *dev_status,
                            ec_stream stream);
/* ec_repair_segments_sets with a stripe count per segment: a repair queue holds
 * segments of as many sizes as there are objects, and one stream-ordered pass
 * serves them all.  Segment g has nstripes[g] stripes: its shares and its
 * outputs are nstripes[g]*ess bytes each.  Everything else is as above: shares,
 * targets and outputs flattened per segment, the basis infectious Rebuild's
 * choice, the rows solved on the host and staged in an event-recycled block,
 * async on stream, no host synchronisation, no caller memory retained.  Each
 * 2048-column tile finds its segment through a per-launch map, as in
 * ec_rebuild_segments_sized; a batch of thousands of segments goes in passes of
 * bounded staging, and a class of more tiles than one launch takes in several
 * launches, so no segment is too long for the call other than by the limit
 * below.
 *
 * Every segment is validated before anything is queued: on an argument error
 * nothing is written and no status word is touched.  The errors are those of
 * ec_repair_segments_sets, and a segment whose nstripes[g]*ess/16 does not fit
 * 32 bits: EC_ERR_UNSUPPORTED.  nstripes[g] == 0 or ntargets[g] == 0 skips
 * segment g: its entries of nums, pieces, targets and outs are stepped over and
 * otherwise not looked at (they may be NULL).  With EC_FLAG_CHECK_SHARES
 * (at most 128 shares per segment) dev_status[g] is as above, and a skipped
 * segment's word is zeroed like the others.
 *
 * Segments whose share size is no multiple of 16, or with a share or output
 * pointer that is not 16-byte aligned, go one by one through the byte kernel
 * with their own stripe count; same results, and the other segments of the
 * call stay in the pass.  Up to k = 128.  Not under stream capture
 * (EC_ERR_UNSUPPORTED). */
int ec_repair_segments_sized(const ec_ctx *ctx, size_t nseg, const int *nshares, const int *nums,
                             const uint8_t *const *pieces, const int *ntargets, const int *targets,
                             uint8_t *const *outs, const size_t *nstripes, int flags, int32_t *dev_status,
                             ec_stream stream);
/* ec_rebuild_segments[_batched] with a share set the context has no
 * straight-line code for runs the share-set pass and has the code made in the
 * background (DESIGN.md §4 "Straight-line rebuild bodies"); later launches of
 * the set use it.  This queues that for (nshares, nums) ahead of time; with
 * wait != 0 it returns after it is made.  Returns 1 when the code is ready, 0
 * when not (or the set has none: every data share present).  No reference
 * counterpart (an engine knob). */
int ec_prepare_rebuild(const ec_ctx *ctx, int nshares, const int *nums, int wait);

/* ---- host-memory pipeline (end-to-end path, PCIe-inclusive) ----
 * Same layouts as the device calls, but in host memory (pinned memory from
 * ec_host_alloc gives full-speed DMA).  Segments are streamed through a ring
 * of device slots on 3 HIP streams so H2D, kernel and D2H of consecutive
 * segments overlap; synchronous (returns when every piece is in host memory).
 * This is the form the Go side calls from segmentupload (SegmentEncoder,
 * single.go:233-238) and StripeReader (BatchRebuilder, stripe.go:382-428). */
int ec_encode_segments_host(const ec_ctx *ctx, const uint8_t *segs, size_t nseg, size_t nstripes, uint8_t *pieces,
                            int flags);
/* pieces[i]: host pointer of share nums[i] for segment 0; segment g's copy of
 * that share is at pieces[i] + g*piece_seg_stride. out: [nseg][stripes*k*ess] */
int ec_rebuild_segments_host(const ec_ctx *ctx, int nshares, const int *nums, const uint8_t *const *pieces,
                             size_t nstripes, size_t nseg, long long piece_seg_stride, uint8_t *out);
/* ec_encode_segments_host + the BLAKE3-256 hash of every piece (all n, also
 * with EC_FLAG_PARITY_ONLY): hashes = [nseg][n][32] host bytes, the value
 * piecestore's upload sends as PieceHash.Hash (piecestore/upload.go:133,155,270)
 * when the piece hash algorithm is BLAKE3 (the default, piecestore/hash.go:20-26). */
int ec_encode_segments_host_hashed(const ec_ctx *ctx, const uint8_t *segs, size_t nseg, size_t nstripes,
                                   uint8_t *pieces, uint8_t *hashes, int flags);
/* Streamed form for one segment, for piece readers that serve each piece
 * stripe by stripe as the reference does (segmentupload/encode.go:39-75,
 * pieceReader.PieceReader single.go:228-238): the segment goes through the
 * engine in chunks of stripes (chunk_stripes, or 0 for the library's choice:
 * 128 stripes first, doubling up to 2048) and each chunk of every piece is in
 * `pieces` (host, [rows][nstripes*ess] as ec_encode_segments_host) as soon as
 * it is encoded.  ec_upload_begin queues everything and returns;
 * ec_upload_wait blocks until stripes [0, stripes) of every piece are in host
 * memory; ec_upload_ready returns how many leading stripes are, without
 * blocking; ec_upload_end waits for the rest, frees the handle and returns the
 * first error.  The caller keeps seg and pieces alive until ec_upload_end.
 * With EC_FLAG_HASH_PIECES the BLAKE3-256 of all n pieces (also with
 * EC_FLAG_PARITY_ONLY) is computed as the chunks stream, as piecestore's
 * upload hashes each piece through a TeeReader (piecestore/upload.go:155,
 * 262-270); ec_upload_hashes waits for them (the last chunk's tree fold) and
 * copies n*32 bytes into `hashes`.  Any number of threads may be inside
 * ec_upload_wait / _ready / _hashes at once; ec_upload_end waits for those
 * inside to return before it frees the handle, and no call may start on a
 * handle once ec_upload_end has been called (callers arriving while it waits
 * get EC_ERR_INVALID_ARG / 0). */
typedef struct ec_upload ec_upload;
int ec_upload_begin(const ec_ctx *ctx, const uint8_t *seg, size_t nstripes, uint8_t *pieces, int flags,
                    size_t chunk_stripes, ec_upload **out);
int ec_upload_wait(ec_upload *u, size_t stripes);
size_t ec_upload_ready(ec_upload *u);
int ec_upload_hashes(ec_upload *u, uint8_t *hashes);
int ec_upload_end(ec_upload *u);
void *ec_host_alloc(size_t bytes); /* pinned (hipHostMalloc); NULL on failure */
void ec_host_free(void *p);
/* Device memory on the current device for the device-pointer calls (the
 * share-set calls' pieces and outputs; a Go binding has no other allocator),
 * and a synchronous copy between any two of host / pinned / device memory. */
void *ec_device_alloc(size_t bytes); /* hipMalloc; NULL on failure */
void ec_device_free(void *p);
int ec_copy(void *dst, const void *src, size_t bytes); /* hipMemcpy(hipMemcpyDefault) */

/* ---- BLAKE3-256 piece hashes (github.com/zeebo/blake3 v0.2.3, go.mod:29) ----
 * Replace the per-piece hash.Hash fed by io.TeeReader during upload
 * (piecestore/upload.go:133 NewHashFromAlgorithm, :155 TeeReader, :270
 * Sum(nil)); 32-byte digests, BLAKE3 hash mode, no key. */

/* Device pieces: byte t of piece j is at
 *   base + j*piece_stride + (t / run)*run_stride + t % run
 * (run = piece_len or 0 for contiguous pieces).  hashes: npieces*32 device
 * bytes.  Async on stream (scratch from hipMallocAsync on that stream). */
int ec_blake3_pieces(const uint8_t *base, size_t npieces, long long piece_stride, size_t piece_len, size_t run,
                     long long run_stride, uint8_t *hashes, ec_stream stream);
/* Every piece of nseg segments already on the device: data piece j of
 * segment s is share j of each stripe of segs + s*nstripes*k*ess; parity
 * piece k+r is parity + (s*(n-k) + r)*nstripes*ess (the EC_FLAG_PARITY_ONLY
 * output).  hashes: [nseg][n][32] device bytes.  Async on stream. */
int ec_hash_segments(const ec_ctx *ctx, const uint8_t *segs, const uint8_t *parity, size_t nseg, size_t nstripes,
                     uint8_t *hashes, ec_stream stream);
/* ---- a length per piece (the hashes of a batch of uploads of different sizes) ----
 * Every piece that goes to a storage node is sent with its hash
 * (piecestore/upload.go:133,155,270), and the uploads in flight at once are of
 * as many sizes as there are objects (single.go:233-238): these two calls hash
 * the pieces of such a batch in one stream-ordered pass, where the calls above
 * take one piece length per call.  One workgroup per 256 KiB of a piece finds
 * its piece through a per-pass map; a piece of up to 256 KiB is finished there,
 * a piece of up to 64 MiB by one more workgroup of a second launch.  A piece
 * whose address and runs allow 16-byte loads takes them whatever the rest of the
 * list looks like (a pass is at most two chunk launches, one per kind, and one
 * parents launch); a piece of more than 64 MiB goes on its own through
 * ec_blake3_pieces' path; same bytes out.  Descriptors, maps and tree nodes are
 * staged in event-recycled blocks of a pool on the context, long lists go in
 * passes of bounded staging, and no caller memory is retained after return.
 * Everything is validated before anything is queued: on an argument error
 * nothing is written.  Async on stream, no host synchronisation once the pool
 * is warm.  Not under stream capture (EC_ERR_UNSUPPORTED). */

/* BLAKE3-256 of npieces contiguous device pieces, piece i at pieces[i] with
 * lens[i] bytes; hashes: npieces*32 device bytes, row i = piece i.
 * lens[i] == 0 gives the hash of the empty input, and pieces[i] may then be
 * NULL; a NULL pieces[i] with lens[i] > 0: EC_ERR_INVALID_ARG.  NULL hashes,
 * pieces or lens with npieces > 0: EC_ERR_INVALID_ARG.  npieces == 0: EC_OK,
 * nothing queued. */
int ec_blake3_pieces_list(const ec_ctx *ctx, size_t npieces, const uint8_t *const *pieces, const size_t *lens,
                          uint8_t *hashes, ec_stream stream);
/* All n piece hashes of a batch encoded by ec_encode_segments_sized: same
 * segs / nstripes / pieces / flags as that call.  hashes: [nseg][n][32] device.
 * Without EC_FLAG_PARITY_ONLY pieces[g] is [n][nstripes[g]*ess] and all n rows
 * are hashed from it; segs may be NULL.  With EC_FLAG_PARITY_ONLY pieces[g] is
 * [n-k][...] and data piece j is read from segs[g] in place (runs of ess bytes,
 * k*ess apart, as ec_hash_segments reads it): segs[g] is required.
 * nstripes[g] == 0 skips segment g: nothing of it is read, its pointers may be
 * NULL and its n*32 hash bytes are left untouched.  A NULL pointer of a segment
 * that is not skipped: EC_ERR_INVALID_ARG. */
int ec_hash_segments_sized(const ec_ctx *ctx, size_t nseg, const uint8_t *const *segs, const size_t *nstripes,
                           const uint8_t *const *pieces, int flags, uint8_t *hashes, ec_stream stream);
/* Launches of the two calls above on this ctx so far (a diagnostic): chunk
 * launches over pieces read with 16-byte loads, chunk launches over pieces read
 * byte by byte, parents launches, and pieces of more than 64 MiB sent through
 * ec_blake3_pieces' path.  Any pointer may be NULL.  No reference counterpart. */
int ec_hash_list_stats(const ec_ctx *ctx, unsigned long long *fast, unsigned long long *bytewise,
                       unsigned long long *parents, unsigned long long *oversize);
/* Host buffers, synchronous: hashes[32*j] = BLAKE3(data + j*stride, piece_len) */
int ec_blake3_host(const uint8_t *data, size_t npieces, long long stride, size_t piece_len, uint8_t *hashes);

/* ---- SHA-256 piece hashes (pb.PieceHashAlgorithm_SHA256, hash.go:15-26) ----
 * The other value of the upload's piece hash algorithm, the protobuf zero value
 * and the legacy one (WithPieceHashAlgo overrides the BLAKE3 default,
 * piecestore/hash.go:20-26; upload.go:133,155,270).  FIPS 180-4, 32-byte
 * digests.  SHA-256 is one serial chain per piece: a piece is one lane of a
 * kernel, so a call is as fast as it has pieces -- one piece is never fast, a
 * batch of segments is thousands of chains.  A launch advances every piece by
 * at most 16,384 blocks (1 MiB), the state carried in device memory between the
 * launches of a call, so every kernel stays short and a piece of any length up
 * to 2^61 - 1 bytes takes the same path (longer: EC_ERR_UNSUPPORTED).  A piece
 * with a 16-byte aligned base and run stride that is contiguous or has runs of
 * a power of two >= 64 bytes is read with 16-byte loads, any other byte by
 * byte; both kinds share a call.
 * The calls have their BLAKE3 siblings' rules: everything is validated before
 * anything is queued, on an argument error nothing is written, async on stream,
 * no caller memory retained; the list calls stage in the same event-recycled
 * pool and are not for a capturing stream (EC_ERR_UNSUPPORTED). */
#define EC_HASH_SHA256 0 /* pb.PieceHashAlgorithm values */
#define EC_HASH_BLAKE3 1

/* SHA-256 of npieces contiguous device pieces, piece i at pieces[i] with
 * lens[i] bytes; hashes: npieces*32 device bytes, row i = piece i.
 * lens[i] == 0 gives the digest of the empty message, and pieces[i] may then be
 * NULL; a NULL pieces[i] with lens[i] > 0: EC_ERR_INVALID_ARG.  NULL hashes,
 * pieces or lens with npieces > 0: EC_ERR_INVALID_ARG.  npieces == 0: EC_OK,
 * nothing queued. */
int ec_sha256_pieces_list(const ec_ctx *ctx, size_t npieces, const uint8_t *const *pieces, const size_t *lens,
                          uint8_t *hashes, ec_stream stream);
/* All n piece hashes of a batch encoded by ec_encode_segments_sized: same
 * segs / nstripes / pieces / flags as that call, and ec_hash_segments_sized's
 * contract.  hashes: [nseg][n][32] device.  With EC_FLAG_PARITY_ONLY data piece
 * j is read from segs[g] in place (runs of ess bytes, k*ess apart).
 * nstripes[g] == 0 skips segment g: its pointers may be NULL and its n*32 hash
 * bytes are left untouched.  A NULL pointer of a segment that is not skipped:
 * EC_ERR_INVALID_ARG. */
int ec_sha256_segments_sized(const ec_ctx *ctx, size_t nseg, const uint8_t *const *segs, const size_t *nstripes,
                             const uint8_t *const *pieces, int flags, uint8_t *hashes, ec_stream stream);
/* Device pieces of one length, addressed as ec_blake3_pieces addresses them:
 * byte t of piece j at base + j*piece_stride + (t / run)*run_stride + t % run
 * (run = piece_len or 0 for contiguous pieces).  hashes: npieces*32 device
 * bytes.  Needs no context; async on stream (pieces of more than 1 MiB take
 * npieces*32 bytes of scratch from hipMallocAsync on that stream). */
int ec_sha256_pieces(const uint8_t *base, size_t npieces, long long piece_stride, size_t piece_len, size_t run,
                     long long run_stride, uint8_t *hashes, ec_stream stream);
/* Host buffers, synchronous: hashes[32*j] = SHA-256(data + j*stride, piece_len) */
int ec_sha256_host(const uint8_t *data, size_t npieces, long long stride, size_t piece_len, uint8_t *hashes);
/* A diagnostic: the blocks one launch of the two list calls advances a piece by
 * on this ctx (0 restores the default, 16,384).  Same digests at any value. */
int ec_sha256_set_launch_blocks(ec_ctx *ctx, size_t blocks);
/* Work of the two list calls on this ctx so far (a diagnostic): pieces read with
 * 16-byte loads, pieces read byte by byte, and kernel launches over them.  Any
 * pointer may be NULL.  No reference counterpart. */
int ec_sha256_list_stats(const ec_ctx *ctx, unsigned long long *fast, unsigned long long *bytewise,
                         unsigned long long *launches);

/* ---- AES-256-GCM segment encryption (storj.io/common/encryption, EncAESGCM) ----
 * Replace encryption.TransformWriterPadded(buf, NewEncrypter(EncAESGCM, key,
 * nonce, BlockSize)) on upload (splitter/splitter.go:156,170) and
 * Transform(rr, NewDecrypter(...)) on download (streams/store.go:354-377):
 * blocks of in_block = BlockSize - 16 plaintext bytes (7408 for BlockSize
 * 29*256, project.go:84), block b sealed under the 12-byte nonce + b
 * (little-endian increment, as calcGCMNonce), written as ciphertext || tag.
 * Padding of the plaintext (PadReader rule) and Unpad are the caller's.
 * in_block must be a multiple of 16, buffers 16-byte aligned. */

/* device bytes of one prepared key */
size_t ec_gcm_key_bytes(void);
/* expands nkeys 32-byte keys (host) into dev_keys (nkeys * ec_gcm_key_bytes()
 * device bytes): round keys + GHASH tables; synchronous */
int ec_gcm_prepare_keys(const uint8_t *keys, size_t nkeys, void *dev_keys, ec_stream stream);
/* plain: [nseg][nblocks*in_block] -> out: [nseg][nblocks*(in_block+16)];
 * segment g uses prepared key g and nonce dev_nonces[12*g..]; async */
int ec_gcm_seal_segments(const uint8_t *plain, size_t nseg, size_t nblocks, size_t in_block, const void *dev_keys,
                         const uint8_t *dev_nonces, uint8_t *out, ec_stream stream);
/* the inverse; dev_status[g] = -1 when every block of segment g verified,
 * else the first block whose tag did not (its plaintext must not be used) */
int ec_gcm_open_segments(const uint8_t *cipher, size_t nseg, size_t nblocks, size_t in_block, const void *dev_keys,
                         const uint8_t *dev_nonces, uint8_t *out, int32_t *dev_status, ec_stream stream);
/* the same with explicit segment strides in bytes (multiples of 16, at least
 * the dense size), e.g. to seal straight into the RS encoder's padded input */
int ec_gcm_seal_segments_strided(const uint8_t *plain, long long plain_seg_stride, size_t nseg, size_t nblocks,
                                 size_t in_block, const void *dev_keys, const uint8_t *dev_nonces, uint8_t *out,
                                 long long out_seg_stride, ec_stream stream);
int ec_gcm_open_segments_strided(const uint8_t *cipher, long long cipher_seg_stride, size_t nseg, size_t nblocks,
                                 size_t in_block, const void *dev_keys, const uint8_t *dev_nonces, uint8_t *out,
                                 long long out_seg_stride, int32_t *dev_status, ec_stream stream);
/* ---- a size per segment (the cipher of a batch of uploads or downloads of different sizes) ----
 * The upload seals each segment through TransformWriterPadded(NewEncrypter(...))
 * (splitter/splitter.go:156,170) and the download opens it through decryptRanger
 * (streams/store.go:347-382), each from its own length, key and nonce; the
 * segments in flight at once are of as many sizes as there are objects.  These
 * two calls run the cipher over such a batch in one stream-ordered pass, where
 * the calls above take one nblocks per call.  Segment g is nblocks[g] dense GCM
 * blocks: sealing reads in_block plaintext bytes per block from plain[g] and
 * writes ciphertext || tag (in_block + 16 bytes per block) to out[g]; opening
 * does the reverse.  Segment g uses prepared key g of dev_keys
 * (ec_gcm_key_bytes() apart) and nonce dev_nonces[12*g..], block b sealed under
 * nonce + b: the same bytes as ec_gcm_seal_segments / ec_gcm_open_segments on
 * each segment alone.  A segment's input and output must not overlap each other
 * or another segment's (the caller's to ensure).  Every segment gets workgroups
 * in proportion to its blocks, at least one and at most one per four blocks, out
 * of the grid the uniform call aims for; a workgroup finds its segment through a
 * per-pass map.  ctx supplies only the device and a staging pool: descriptors
 * and maps are staged in event-recycled blocks, long lists go in passes of at
 * most 4096 segments, and no caller memory is retained after return.
 * nblocks[g] == 0 skips segment g: nothing of it is read or written and its
 * pointers may be NULL (the open call still writes dev_status[g] = -1).
 * Everything is validated before anything is queued: on an argument error
 * nothing is written.  EC_ERR_INVALID_ARG: NULL ctx, a NULL array with nseg > 0,
 * NULL dev_keys or dev_nonces, NULL dev_status (open), a NULL pointer of a
 * segment that is not skipped, a data_len that does not pad to nblocks.
 * EC_ERR_UNSUPPORTED: in_block 0, above 1<<24 or no multiple of 16, a pointer
 * of a segment that is not skipped that is not 16-byte aligned, nblocks[g] above
 * 0x7FFFFFFF, nseg above 0xFFFFFFFF, a capturing stream.  nseg == 0: EC_OK,
 * nothing queued.  Async on stream, no host synchronisation once the pool is
 * warm. */

/* data_len NULL: the plaintext is already padded and is only read.  Otherwise
 * segment g holds data_len[g] bytes and the call writes PadReader's padding to
 * in_block behind them, in stream order before the seal -- the bytes
 * ec_pad_segments(plain[g], 1, 0, data_len[g], in_block, stream) writes -- and
 * requires nblocks[g]*in_block == data_len[g] + p,
 * p = 4 + (in_block - (data_len[g]+4) % in_block) % in_block. */
int ec_gcm_seal_segments_sized(const ec_ctx *ctx, size_t nseg, uint8_t *const *plain, const size_t *nblocks,
                               const size_t *data_len /* may be NULL */, size_t in_block, const void *dev_keys,
                               const uint8_t *dev_nonces, uint8_t *const *out, ec_stream stream);
/* dev_status: [nseg] device; dev_status[g] ends as -1, or as the first block of
 * segment g whose tag did not verify (its plaintext must not be used).  A
 * failing segment does not stop the others. */
int ec_gcm_open_segments_sized(const ec_ctx *ctx, size_t nseg, const uint8_t *const *cipher, const size_t *nblocks,
                               size_t in_block, const void *dev_keys, const uint8_t *dev_nonces,
                               uint8_t *const *out, int32_t *dev_status, ec_stream stream);
/* Cipher launches of the two calls above on this ctx so far (a diagnostic): of
 * the seal, of the open, and the passes of both.  Any pointer may be NULL.  No
 * reference counterpart. */
int ec_gcm_sized_stats(const ec_ctx *ctx, unsigned long long *seal_launches, unsigned long long *open_launches,
                       unsigned long long *passes);
/* ---- byte ranges of many segments opened at once (ranged downloads) ----
 * uplink's Download takes an offset and a length, and the range narrows at every
 * layer: decryptRanger's Range (streams/store.go:347-382, encryption.Transform)
 * asks for the cipher blocks CalcEncompassingBlocks(offset, length, in_block)
 * gives, opens block b under nonce + b for the segment's absolute block
 * numbers, discards the head of the first block and limits the length;
 * decodedRanger.Range (eestream/decode.go:199-227) does the same one level down
 * with the stripes that cover those blocks.  This call is the cipher's part for
 * a batch of such ranges in one stream-ordered pass.  Segment g is the
 * nblocks[g] covered blocks first_block[g] .. first_block[g] + nblocks[g] - 1 of
 * its download's segment: cipher[g] holds exactly those blocks, dense,
 * nblocks[g] * (in_block + 16) bytes, and out[g] receives the length[g]
 * plaintext bytes that start head[g] bytes into the first of them -- exactly
 * length[g] bytes, nothing before or after.  cipher[g] and out[g] may have any
 * alignment: the path where both and head[g] are multiples of 16 is the sized
 * open's 16-byte loads and stores, everything else reads and writes narrower.
 * Relative block r is opened under nonce dev_nonces[12*g..] + (first_block[g] + r)
 * with prepared key g of dev_keys, so a caller uses the same key and nonce
 * arrays for a whole open and for any range of it.  Every covered block is
 * authenticated in full, the parts the range does not want included:
 * dev_status[g] ends as -1, or as the smallest absolute block number among the
 * covered blocks whose tag did not verify (the plaintext must then not be used).
 * nblocks[g] == 0 requires length[g] == 0: the segment is skipped, its pointers
 * may be NULL and its status is -1.  Staging, passes of at most 4096 segments,
 * workgroups in proportion to blocks and "everything validated before anything
 * is queued" are as in ec_gcm_open_segments_sized.  EC_ERR_INVALID_ARG: NULL ctx,
 * a NULL array with nseg > 0, NULL dev_keys, dev_nonces or dev_status, a NULL
 * pointer of a segment that is not skipped, head[g] >= in_block, an nblocks[g]
 * that is not the count CalcEncompassingBlocks(head[g], length[g], in_block)
 * gives.  EC_ERR_UNSUPPORTED: in_block 0, above 1<<24 or no multiple of 16,
 * first_block[g] + nblocks[g] above 0x7FFFFFFF (status words are int32), nseg
 * above 0xFFFFFFFF, a capturing stream.  nseg == 0: EC_OK, nothing queued.
 * Async on stream.  (The whole-segment encryption.Decrypt branch of
 * decryptRanger, store.go:360-375, is for inline segments, which never reach
 * the erasure path: that one is ec_gcm_open_messages below.) */
int ec_gcm_open_ranges_sized(const ec_ctx *ctx, size_t nseg, const uint8_t *const *cipher,
                             const size_t *first_block, const size_t *nblocks, const size_t *head,
                             const size_t *length, size_t in_block, const void *dev_keys,
                             const uint8_t *dev_nonces, uint8_t *const *out, int32_t *dev_status, ec_stream stream);
/* Cipher launches of the call above on this ctx so far, and its passes (a
 * diagnostic; ec_gcm_sized_stats does not count them).  Either pointer may be
 * NULL.  No reference counterpart. */
int ec_gcm_ranged_stats(const ec_ctx *ctx, unsigned long long *open_launches, unsigned long long *passes);
/* ---- one-shot messages, a raw key each (inline segments, content keys, metadata) ----
 * Beside the block transform the stream layer calls the cipher in a second
 * form, aesgcm.Seal(nil, nonce[:12], data, nil) over one whole message with no
 * block framing and no padding:
 *   encryption.Encrypt(inline, cipher, &contentKey, &nonce) for an object of up
 *     to maxInlineSize = 4096 bytes, which is never erasure coded
 *     (splitter/splitter.go:189, project.go:24), and encryption.Decrypt of it,
 *     the whole-segment branch of decryptRanger (streams/store.go:360-375);
 *   encryption.EncryptKey / DecryptKey, a 32-byte key sealed to 48 bytes: every
 *     segment's content key (splitter.go:160, store.go:349) and the metadata key
 *     (uploader.go:415, metaclient/objects.go:169,897,1105, move.go:110-154);
 *   Encrypt / Decrypt of stream info and ETags (uploader.go:421,438,
 *     objects.go:1111,1122, multipart_iterators.go:366).
 * These two calls do that for a list of messages in one stream-ordered pass.
 * Message i is len[i] plaintext bytes (0 .. 1<<24) under the 32 raw key bytes
 * dev_keys32[32*i ..] and the nonce dev_nonces[12*i ..], both in device memory at
 * any alignment: J0 = nonce || 00000001, the counter runs from 2, GHASH over the
 * zero-padded ciphertext and the length block with no AAD, tag = GHASH ^
 * AES_K(J0).  len[i] is the plaintext length in both calls; the sealed form is
 * len[i] + 16 bytes, ciphertext || tag.  Everything is derived from the key bytes
 * on the GPU: there is no ec_gcm_prepare_keys and no prepared-key buffer here.
 * plain[i], cipher[i] and out[i] may have any alignment (16-byte loads and
 * stores where an address allows them, narrower ones otherwise); a message's
 * input and output must not overlap each other or another message's.
 * len[i] == 0 is a real message: the seal writes its 16-byte tag, the open
 * checks it; plain[i] of the seal and out[i] of the open may then be NULL.
 * The open authenticates a message before it releases anything of it:
 * dev_status[i] ends as 0, or as 1 when the tag does not verify, and then
 * exactly len[i] zero bytes are written to out[i] (Go's Open leaves no plaintext
 * behind).  A failing message does not disturb the others.
 * One wave of the GPU takes one message, so the calls are for many short
 * messages; a long one is correct (its wave's 64 lanes share it) but gets no
 * more than that wave.  ctx supplies only the device and a staging pool:
 * descriptors are staged in event-recycled blocks in passes of a fixed number of
 * messages (ec_gcm_messages_stats), and no caller memory is retained after
 * return.  Everything is validated before anything is queued: on an error
 * nothing is written.  EC_ERR_INVALID_ARG: NULL ctx, a NULL array with nmsg > 0,
 * NULL dev_keys32 or dev_nonces, NULL dev_status (open), a NULL pointer of a
 * message other than the two len[i] == 0 cases above.  EC_ERR_UNSUPPORTED:
 * len[i] above 1<<24, nmsg above 0xFFFFFFFF, a capturing stream.  nmsg == 0:
 * EC_OK, nothing queued.  Async on stream, no host synchronisation once the
 * pool is warm. */
int ec_gcm_seal_messages(const ec_ctx *ctx, size_t nmsg, const uint8_t *const *plain, const size_t *len,
                         const uint8_t *dev_keys32, const uint8_t *dev_nonces, uint8_t *const *out, ec_stream stream);
int ec_gcm_open_messages(const ec_ctx *ctx, size_t nmsg, const uint8_t *const *cipher, const size_t *len,
                         const uint8_t *dev_keys32, const uint8_t *dev_nonces, uint8_t *const *out,
                         int32_t *dev_status, ec_stream stream);
/* Cipher launches of the two calls above on this ctx so far (a diagnostic): of
 * the seal, of the open, the passes of both, and the messages a pass holds (a
 * constant of the build).  Any pointer may be NULL.  No reference counterpart. */
int ec_gcm_messages_stats(const ec_ctx *ctx, unsigned long long *seal_launches, unsigned long long *open_launches,
                          unsigned long long *passes, unsigned long long *pass_messages);
/* PadReader padding (single.go:236) on the device: after
 * data_len bytes of each of nseg segments (seg_stride apart) write
 * p = 4 + (block - (data_len+4) % block) % block bytes of byte(p), the last
 * four the big-endian uint32 p.  Async on stream. */
int ec_pad_segments(uint8_t *segs, size_t nseg, long long seg_stride, size_t data_len, size_t block, ec_stream stream);
/* host buffers, one segment, synchronous; open returns EC_ERR_AUTH and the
 * first failing block in *bad_block when a tag does not verify */
int ec_gcm_seal_host(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *plain, size_t nblocks,
                     size_t in_block, uint8_t *out);
int ec_gcm_open_host(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *cipher, size_t nblocks,
                     size_t in_block, uint8_t *out, long long *bad_block);

/* ---- on-box ceilings (the bench's roofline context; no reference counterpart) ----
 * A plain streaming kernel, no arithmetic, in the read:write mix of an erasure
 * kernel: each wave reads R KiB of src and writes W KiB to dst, one-shot grid,
 * 16 B per lane per access (DESIGN.md §4 HBM table).  dst must hold
 * read_bytes * W / R bytes.  *moved = the bytes read + written.  Async. */
#define EC_PROBE_COPY 0       /* 1 : 1     (the rebuild) */
#define EC_PROBE_ENCODE_MIX 1 /* 4 : 11    (the full encode's 29 : 80) */
#define EC_PROBE_PARITY_MIX 2 /* 4 : 7     (the parity-only encode's 29 : 51) */
int ec_bw_probe(int shape, const uint8_t *src, size_t read_bytes, uint8_t *dst, size_t *moved, ec_stream stream);
/* The RS(29,80) encoder's own memory schedule without its arithmetic: exactly
 * ec_encode_segments' launch (same loaders, LDS ring, tile queue, slicing,
 * copy-through and parity stores, flags as there), with the GF
 * multiply-accumulate removed -- each parity row stored is a copy of the
 * tile's last input share, so the pieces written are NOT the code's.  The
 * on-box ceiling of the encoder's access pattern (bench.py); measurement only.
 * EC_ERR_UNSUPPORTED for any other (k, n), or ess / pointers not 16-aligned. */
int ec_encode_shape_probe(const ec_ctx *ctx, const uint8_t *segs, size_t nseg, size_t nstripes, uint8_t *pieces,
                          int flags, ec_stream stream);

/* ---- device helpers ---- */
int ec_device_count(void);
int ec_set_device(int device);
/* name of the kernel ec_encode_segments uses for whole segments of this ctx
 * right now: "straight-line" (at most 32 parity rows: the runtime-matrix
 * kernel with the parity rows as generated straight-line code, unless
 * ec_set_body selected the jump table), "special" (compile-time G, built into
 * the library), "special-jit" (compiled for this (k, n) at run time),
 * "generic" (runtime matrix), "bytes" (ess not a multiple of 16) or "copy"
 * (n == k) */
const char *ec_encode_kernel_name(const ec_ctx *ctx);
/* The compile-time-G encoder of a (k, n) that is not built into the library
 * is compiled in the background from its first whole-segment encode call (at
 * least 256 tiles: a few MiB of stripes) or this call on (hiprtc, ~1 s; the
 * code object is cached on disk); per-stripe and few-stripe calls never start
 * one.  Until it is ready the encode calls use the runtime-matrix kernel, with
 * identical results.  A process that started a compile waits at exit for the
 * one in progress.  Returns 1 when it is ready (with wait != 0: after waiting
 * for the compilation), 0 when this (k, n) has none.  UPLINK_EC_JIT=0 in the
 * environment turns run-time compilation off. */
int ec_prepare_encoder(const ec_ctx *ctx, int wait);
/* Body of the runtime-matrix kernel for this ctx's decode (and other
 * runtime-matrix) plans, DESIGN.md §4 "Straight-line rebuild":
 *   EC_BODY_AUTO (default): the plan's generated straight-line code for
 *     launches of at least 64 tiles (131,072 byte columns per share), the
 *     jump table for smaller ones (per-stripe calls);
 *   EC_BODY_JUMP_TABLE: always the jump table;
 *   EC_BODY_STRAIGHT_LINE: generated code for every launch it fits, and
 *     every encode on it (also those a compile-time encoder would take).
 * The results are identical.  No reference counterpart (an engine knob). */
#define EC_BODY_AUTO 0
#define EC_BODY_JUMP_TABLE 1
#define EC_BODY_STRAIGHT_LINE 2
int ec_set_body(ec_ctx *ctx, int body);
/* which body the ctx's last runtime-matrix launch used: EC_BODY_JUMP_TABLE,
 * EC_BODY_STRAIGHT_LINE, or EC_BODY_AUTO when there was none yet */
int ec_last_body(const ec_ctx *ctx);
/* Compile-time encoder launches of this ctx so far that took a work-counter
 * slot (tiles handed out by a queue) and that assigned their tiles statically
 * because no slot was free without waiting for another stream (identical
 * results; a diagnostic).  No reference counterpart. */
int ec_encoder_queue_stats(const ec_ctx *ctx, unsigned long long *queued, unsigned long long *static_tiles);
/* Identity of this build: 16 hex digits of a SHA-256 over the library's
 * sources, generators and build flags (uplink_amd/csrc/Makefile).  Measurement
 * records taken from one build (profiles/pmc_traffic.json) carry it, so a bench
 * run of another build can tell they are stale.  No reference counterpart. */
const char *ec_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* UPLINK_EC_H */
