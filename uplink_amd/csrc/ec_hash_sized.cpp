// C-ABI, BLAKE3 piece hashes of pieces that each have their own length
// (include/uplink_ec.h ec_blake3_pieces_list, ec_hash_segments_sized): the hash
// every piece is sent with (piecestore/upload.go:133,155,270) for a batch of
// uploads of as many sizes as objects, in one stream-ordered pass.  The host
// validates every piece, classifies it (fast / byte / oversize), lays each pass
// out (b3_list_geom.hpp) and stages descriptors, maps and node scratch in
// event-recycled blocks, as the sized encode does (ec_encode_sized.cpp); nothing
// on the call path waits for the stream.
#include "b3_list_geom.hpp"
#include "ec_internal.hpp"
#include "hash_list.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One pass over pieces[0..n) (classes cls): staging, then at most two chunk
// launches and one parents launch on s.
int hash_list_pass(ec_ctx *c, const HashPiece *pieces, const b3list::Class *cls, size_t n, uint8_t *hash_lo,
                   uint8_t *hash_hi, hipStream_t s) {
    std::vector<b3list::Piece> ps(n);
    for (size_t i = 0; i < n; i++) ps[i] = pieces[i].p;
    const b3list::Layout L = b3list::layout(ps.data(), cls, n);
    if (L.wgs[0] + L.wgs[1] == 0) return EC_OK;  // (oversize pieces only)
    const size_t desc_bytes = up(n * sizeof(B3ListDesc), 256), map_bytes = up(L.map.size() * 4, 256),
                 par_bytes = up(L.parents.size() * 4, 256);
    const size_t stage_bytes = desc_bytes + map_bytes + par_bytes;
    StageBlock *b = block_acquire(c->hash_sized, stage_bytes, stage_bytes + (size_t)L.nodes * 32);
    if (!b) return EC_ERR_DEVICE;
    B3ListDesc *hd = (B3ListDesc *)b->h;
    for (size_t i = 0; i < n; i++) {
        const b3list::Run r = b3list::run_of(ps[i]);
        B3ListDesc &d = hd[i];
        d.base = (const uint8_t *)(uintptr_t)ps[i].base;
        d.len = ps[i].len;
        d.run = r.run;
        d.run_stride = r.run_stride;
        d.hash = pieces[i].hash;
        d.wg0 = L.wg0[i];
        d.node0 = L.node0[i];
        d.groups = L.groups[i];
        d.run_shift = r.run_shift;
        d.rsv = 0;
    }
    if (!L.map.empty()) memcpy(b->h + desc_bytes, L.map.data(), L.map.size() * 4);
    if (!L.parents.empty()) memcpy(b->h + desc_bytes + map_bytes, L.parents.data(), L.parents.size() * 4);
    B3ListPass p{};
    p.h_stage = b->h;
    p.d_stage = b->d;
    p.stage_bytes = stage_bytes;
    p.desc = (const B3ListDesc *)b->d;
    p.map_fast = (const uint32_t *)(b->d + desc_bytes);
    p.map_byte = p.map_fast + L.wgs[0];
    p.parents = (const uint32_t *)(b->d + desc_bytes + map_bytes);
    p.wgs_fast = L.wgs[0];
    p.wgs_byte = L.wgs[1];
    p.nparents = (uint32_t)L.parents.size();
    p.nodes = (uint32_t *)(b->d + stage_bytes);
    p.node_cap = L.nodes;
    p.hash_lo = hash_lo;
    p.hash_hi = hash_hi;
    p.chk_flag = c->d_chk;
    const hipError_t e = b3_launch_list(p, s);
    // (a failed launch may have queued the launches before it: the block waits for the stream)
    block_release(c->hash_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    if (p.wgs_fast) c->hl_fast.fetch_add(1, std::memory_order_relaxed);
    if (p.wgs_byte) c->hl_byte.fetch_add(1, std::memory_order_relaxed);
    if (p.nparents) c->hl_parents.fetch_add(1, std::memory_order_relaxed);
    return after_launch(c->d_chk, s);
}

// A piece of more than 256 groups, on its own through the uniform launch: same bytes out.
int hash_oversize(ec_ctx *c, const HashPiece &hp, hipStream_t s) {
    const B3View v{(const uint8_t *)(uintptr_t)hp.p.base, 0, hp.p.len, hp.p.run, hp.p.run_stride, 1, 0, 0, 0};
    const size_t ws_bytes = b3_workspace_bytes(v);
    void *ws = nullptr;
    if (ws_bytes) HIP_TRY(hipMallocAsync(&ws, ws_bytes, s));
    const hipError_t e = b3_launch(v, hp.hash, ws, s);
    if (ws) (void)hipFreeAsync(ws, s);
    c->hl_oversize.fetch_add(1, std::memory_order_relaxed);
    return hip_fail(e);
}

// pieces: validated, none of them retained.  [hash_lo, hash_hi): the caller's hash buffer.
int hash_list(ec_ctx *c, const std::vector<HashPiece> &pieces, uint8_t *hash_lo, uint8_t *hash_hi, hipStream_t s) {
    if (pieces.empty()) return EC_OK;
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    std::vector<b3list::Piece> ps(pieces.size());
    std::vector<b3list::Class> cls(pieces.size());
    for (size_t i = 0; i < pieces.size(); i++) {
        ps[i] = pieces[i].p;
        cls[i] = b3list::classify(ps[i]);
    }
    for (const sized::Pass &p : b3list::split(ps.data(), cls.data(), ps.size()))
        if (int rc = hash_list_pass(c, pieces.data() + p.i0, cls.data() + p.i0, p.i1 - p.i0, hash_lo, hash_hi, s))
            return rc;
    for (size_t i = 0; i < pieces.size(); i++)
        if (cls[i] == b3list::kOversize)
            if (int rc = hash_oversize(c, pieces[i], s)) return rc;
    return EC_OK;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_blake3_pieces_list(const ec_ctx *cc, size_t npieces, const uint8_t *const *pieces, const size_t *lens,
                          uint8_t *hashes, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (npieces && (!pieces || !lens || !hashes))) return EC_ERR_INVALID_ARG;
    if (npieces == 0) return EC_OK;
    // every piece is validated before anything is queued
    std::vector<HashPiece> list;
    if (int rc = list_pieces(npieces, pieces, lens, hashes, list)) return rc;
    DeviceGuard dg(c->device);
    return hash_list(c, list, hashes, hashes + 32 * npieces, (hipStream_t)stream);
}

int ec_hash_segments_sized(const ec_ctx *cc, size_t nseg, const uint8_t *const *segs, const size_t *nstripes,
                           const uint8_t *const *pieces, int flags, uint8_t *hashes, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nstripes || !pieces || !hashes))) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    // every segment is validated before anything is queued
    std::vector<HashPiece> list;
    if (int rc = segment_pieces(c, nseg, segs, nstripes, pieces, flags, hashes, list)) return rc;
    DeviceGuard dg(c->device);
    return hash_list(c, list, hashes, hashes + 32 * (size_t)c->n * nseg, (hipStream_t)stream);
}

int ec_hash_list_stats(const ec_ctx *c, unsigned long long *fast, unsigned long long *bytewise,
                       unsigned long long *parents, unsigned long long *oversize) {
    if (!c) return EC_ERR_INVALID_ARG;
    if (fast) *fast = c->hl_fast.load(std::memory_order_relaxed);
    if (bytewise) *bytewise = c->hl_byte.load(std::memory_order_relaxed);
    if (parents) *parents = c->hl_parents.load(std::memory_order_relaxed);
    if (oversize) *oversize = c->hl_oversize.load(std::memory_order_relaxed);
    return EC_OK;
}

}  // extern "C"
