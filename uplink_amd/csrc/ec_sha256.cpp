// C-ABI, SHA-256 piece hashes (include/uplink_ec.h ec_sha256_*): the hash every
// piece is sent with when the upload was opened with pb.PieceHashAlgorithm_SHA256
// (piecestore/hash.go:15-26, upload.go:133,155,270).  The list calls validate every
// piece, lay each pass out one lane per piece (sha_list_geom.hpp), stage the
// descriptors and keep the carried state in an event-recycled block of the pool
// the BLAKE3 list calls use (ec_hash_sized.cpp), and queue the pass's launches;
// nothing on the call path waits for the stream.
#include "ec_internal.hpp"
#include "hash_list.hpp"
#include "sha256.hpp"
#include "sha_list_geom.hpp"

namespace uplink_ec {
namespace capi {
namespace {

uint64_t launch_blocks_of(const ec_ctx *c) {
    const uint64_t b = c->sha_launch_blocks.load(std::memory_order_relaxed);
    return b ? b : shalist::kLaunchBlocks;
}

// One pass over pieces[0..n): staging, then its launches on s.
int sha_list_pass(ec_ctx *c, const HashPiece *pieces, size_t n, uint8_t *hash_lo, uint8_t *hash_hi, hipStream_t s) {
    std::vector<b3list::Piece> ps(n);
    for (size_t i = 0; i < n; i++) ps[i] = pieces[i].p;
    const shalist::Layout L = shalist::layout(ps.data(), n);
    const size_t desc_bytes = up((size_t)L.lanes() * sizeof(ShaDesc), 256);
    StageBlock *b = block_acquire(c->hash_sized, desc_bytes, desc_bytes + (size_t)L.lanes() * 32);
    if (!b) return EC_ERR_DEVICE;
    ShaDesc *hd = (ShaDesc *)b->h;
    memset(hd, 0, desc_bytes);  // (a padding lane: hash == nullptr)
    for (uint32_t j = 0; j < L.lanes(); j++) {
        if (L.row[j] == shalist::kNone) continue;
        const b3list::Piece &p = ps[L.row[j]];
        const b3list::Run r = b3list::run_of(p);
        ShaDesc &d = hd[j];
        d.base = (const uint8_t *)(uintptr_t)p.base;
        d.len = p.len;
        d.run = r.run;
        d.run_stride = r.run_stride;
        d.hash = pieces[L.row[j]].hash;
        d.run_shift = r.run_shift;
        d.fast = shalist::class_of(p) == shalist::kFast;
    }
    ShaListPass p{};
    p.h_stage = b->h;
    p.d_stage = b->d;
    p.stage_bytes = desc_bytes;
    p.desc = (const ShaDesc *)b->d;
    p.lanes = L.lanes();
    p.state = (uint32_t *)(b->d + desc_bytes);
    p.launch_blocks = launch_blocks_of(c);
    p.launches = shalist::launches_of(L.max_blocks, p.launch_blocks);
    p.hash_lo = hash_lo;
    p.hash_hi = hash_hi;
    p.chk_flag = c->d_chk;
    const hipError_t e = sha256_launch_list(p, s);
    // (a failed launch may have queued the launches before it: the block waits for the stream)
    block_release(c->hash_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    c->sha_fast.fetch_add(L.count[shalist::kFast], std::memory_order_relaxed);
    c->sha_byte.fetch_add(L.count[shalist::kByte], std::memory_order_relaxed);
    c->sha_launches.fetch_add(p.launches, std::memory_order_relaxed);
    return after_launch(c->d_chk, s);
}

// pieces: validated, none of them retained.  [hash_lo, hash_hi): the caller's hash buffer.
int sha_list(ec_ctx *c, const std::vector<HashPiece> &pieces, uint8_t *hash_lo, uint8_t *hash_hi, hipStream_t s) {
    if (pieces.empty()) return EC_OK;
    for (const HashPiece &hp : pieces)
        if (hp.p.len > shalist::kMaxLen) return EC_ERR_UNSUPPORTED;
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    for (const sized::Pass &p : shalist::split(pieces.size()))
        if (int rc = sha_list_pass(c, pieces.data() + p.i0, p.i1 - p.i0, hash_lo, hash_hi, s)) return rc;
    return EC_OK;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_sha256_pieces_list(const ec_ctx *cc, size_t npieces, const uint8_t *const *pieces, const size_t *lens,
                          uint8_t *hashes, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (npieces && (!pieces || !lens || !hashes))) return EC_ERR_INVALID_ARG;
    if (npieces == 0) return EC_OK;
    // every piece is validated before anything is queued
    std::vector<HashPiece> list;
    if (int rc = list_pieces(npieces, pieces, lens, hashes, list)) return rc;
    DeviceGuard dg(c->device);
    return sha_list(c, list, hashes, hashes + 32 * npieces, (hipStream_t)stream);
}

int ec_sha256_segments_sized(const ec_ctx *cc, size_t nseg, const uint8_t *const *segs, const size_t *nstripes,
                             const uint8_t *const *pieces, int flags, uint8_t *hashes, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nstripes || !pieces || !hashes))) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    // every segment is validated before anything is queued
    std::vector<HashPiece> list;
    if (int rc = segment_pieces(c, nseg, segs, nstripes, pieces, flags, hashes, list)) return rc;
    DeviceGuard dg(c->device);
    return sha_list(c, list, hashes, hashes + 32 * (size_t)c->n * nseg, (hipStream_t)stream);
}

int ec_sha256_pieces(const uint8_t *base, size_t npieces, long long piece_stride, size_t piece_len, size_t run,
                     long long run_stride, uint8_t *hashes, ec_stream stream) {
    if (!hashes || (!base && piece_len && npieces)) return EC_ERR_INVALID_ARG;
    if (npieces == 0) return EC_OK;
    if (piece_len > shalist::kMaxLen) return EC_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const ShaView v{base, piece_stride, piece_len, run, run_stride, npieces};
    void *state = nullptr;  // carried between launches; none when one launch finishes the pieces
    if (sha256_uniform_launches(v, shalist::kLaunchBlocks) > 1) {
        if (npieces > SIZE_MAX / 32) return EC_ERR_INVALID_ARG;
        HIP_TRY(hipMallocAsync(&state, 32 * npieces, st));
    }
    const hipError_t e = sha256_launch_uniform(v, hashes, (uint32_t *)state, shalist::kLaunchBlocks, st);
    if (state) (void)hipFreeAsync(state, st);
    return hip_fail(e);
}

int ec_sha256_host(const uint8_t *data, size_t npieces, long long stride, size_t piece_len, uint8_t *hashes) {
    if (!hashes || (!data && piece_len && npieces)) return EC_ERR_INVALID_ARG;
    if (npieces == 0) return EC_OK;
    const size_t span = (npieces - 1) * (size_t)stride + piece_len;
    hipStream_t st = nullptr;
    uint8_t *d = nullptr;
    int rc = EC_OK;
    do {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { rc = EC_ERR_DEVICE; break; }
        if (hipMalloc(&d, up(span, 256) + 32 * npieces) != hipSuccess) { rc = EC_ERR_DEVICE; d = nullptr; break; }
        uint8_t *dh = d + up(span, 256);
        if (span && hipMemcpyAsync(d, data, span, hipMemcpyHostToDevice, st) != hipSuccess) { rc = EC_ERR_DEVICE; break; }
        rc = ec_sha256_pieces(d, npieces, stride, piece_len, piece_len, stride, dh, st);
        if (rc) break;
        if (hipMemcpyAsync(hashes, dh, 32 * npieces, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = EC_ERR_DEVICE; break; }
        if (hipStreamSynchronize(st) != hipSuccess) rc = EC_ERR_DEVICE;
    } while (0);
    if (st) (void)hipStreamSynchronize(st);
    if (d) (void)hipFree(d);
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

int ec_sha256_set_launch_blocks(ec_ctx *c, size_t blocks) {
    if (!c) return EC_ERR_INVALID_ARG;
    c->sha_launch_blocks.store(blocks, std::memory_order_relaxed);
    return EC_OK;
}

int ec_sha256_list_stats(const ec_ctx *c, unsigned long long *fast, unsigned long long *bytewise,
                         unsigned long long *launches) {
    if (!c) return EC_ERR_INVALID_ARG;
    if (fast) *fast = c->sha_fast.load(std::memory_order_relaxed);
    if (bytewise) *bytewise = c->sha_byte.load(std::memory_order_relaxed);
    if (launches) *launches = c->sha_launches.load(std::memory_order_relaxed);
    return EC_OK;
}

}  // extern "C"
