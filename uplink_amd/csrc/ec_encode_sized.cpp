// C-ABI, encode with a size per segment (include/uplink_ec.h
// ec_encode_segments_sized): a batch of uploads of as many sizes as objects,
// each padded (when given by its data length) and encoded into its own pieces,
// in one stream-ordered pass (rs_encode_sized.hpp).  The host validates every
// segment, lays the pass's blocks out (enc_sized_geom.hpp) and stages one
// record per segment in event-recycled blocks, as the sized share-set calls do
// (ec_sized.cpp); nothing on the call path waits for the stream.
#include "ec_internal.hpp"
#include "enc_sized_geom.hpp"
#include "rs_encode_sized.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One segment the sized kernel takes.
struct EncSeg {
    const uint8_t *in;
    uint8_t *out;
    int64_t nstripes, chunks, blocks;
    uint64_t data_len;
    uint32_t pad;  // 0: already padded
};

// One pass over segs[0..n): rs_encode_sized_prep, then the encoder, on stream s.
int encode_sized_pass(ec_ctx *c, const EncoderKernel &ek, const EncSeg *segs, size_t n, bool parity_only,
                      hipStream_t s) {
    std::vector<int64_t> blocks(n), block0(n);
    for (size_t i = 0; i < n; i++) blocks[i] = segs[i].blocks;
    const int64_t B = sized::first_blocks(blocks.data(), n, block0.data());
    const size_t d_desc = up(n * sizeof(EncSizedDesc), 256), d_map = up((size_t)B * 4, 256);
    StageBlock *b = block_acquire(c->enc_sized, n * sizeof(EncSizedStage), d_desc + d_map);
    if (!b) return EC_ERR_DEVICE;
    EncSizedStage *stage = (EncSizedStage *)b->h;
    EncSizedDesc *d_descs = (EncSizedDesc *)b->d;
    uint32_t *map = (uint32_t *)(b->d + d_desc);
    for (size_t i = 0; i < n; i++) {
        EncSizedStage &st = stage[i];
        st.d.in = segs[i].in;
        st.d.out = segs[i].out;
        st.d.chunks = segs[i].chunks;
        st.d.piece_len = segs[i].nstripes * c->ess;
        st.d.block0 = block0[i];
        st.nblocks = segs[i].blocks;
        st.data_len = segs[i].data_len;
        st.pad = segs[i].pad;
        st.rsv = 0;
    }
    hipError_t e = launch_encode_sized_prep(stage, d_descs, map, (int)n, s);
    if (e != hipSuccess) {  // nothing was queued
        block_release(c->enc_sized, b, false, s);
        return hip_fail(e);
    }
    EncSizedArgs a{};
    a.desc = d_descs;
    a.map = map;
    a.total_blocks = B;
    a.ess = c->ess;
    a.cps = c->ess / 16;
    a.chk_flag = c->d_chk;
    int slot = -1;
    a.queue = queue_take(c, s, &slot, &a.queue_seq, &a.queue_host_done);
    (a.queue ? c->q_taken : c->q_static).fetch_add(1, std::memory_order_relaxed);
    e = launch_encode_sized(ek, a, parity_only, 0, s);
    if (slot >= 0) queue_done(c, s, slot, a.queue_seq, e == hipSuccess);
    block_release(c->enc_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    return after_launch(c->d_chk, s);
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_encode_segments_sized(const ec_ctx *cc, size_t nseg, uint8_t *const *segs, const size_t *nstripes,
                             const size_t *data_len, uint8_t *const *pieces, int flags, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!segs || !nstripes || !pieces))) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    const int k = c->k, n = c->n, ess = c->ess;
    if (k > kMaxOps) return EC_ERR_UNSUPPORTED;
    DeviceGuard dg(c->device);
    hipStream_t s = (hipStream_t)stream;
    const bool parity_only = (flags & EC_FLAG_PARITY_ONLY) != 0;
    const uint64_t stripe = (uint64_t)k * ess;
    // the library-built encoder of this code, if any: this call starts no run-time compile
    const EncoderKernel *ek = n > k && ess % 16 == 0 ? aot_encoder(k, n) : nullptr;
    // every segment is validated before anything is queued
    std::vector<EncSeg> fast;
    std::vector<size_t> own;  // segments the existing path takes, one by one
    for (size_t g = 0; g < nseg; g++) {
        if (nstripes[g] == 0) continue;
        if (!segs[g] || !pieces[g]) return EC_ERR_INVALID_ARG;
        const int64_t chunks = sized::chunks_of(nstripes[g], ess);
        if (chunks < 0) return EC_ERR_UNSUPPORTED;
        uint32_t pad = 0;
        if (data_len) {
            if (!sized::pad_matches(data_len[g], nstripes[g], stripe)) return EC_ERR_INVALID_ARG;
            pad = (uint32_t)sized::pad_amount(data_len[g], stripe);
        }
        if (ek && aligned16(segs[g]) && aligned16(pieces[g]))
            fast.push_back({segs[g], pieces[g], (int64_t)nstripes[g], chunks, sized::blocks_of(chunks),
                            data_len ? (uint64_t)data_len[g] : 0, pad});
        else
            own.push_back(g);
    }
    if (fast.empty() && own.empty()) return EC_OK;
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    // another (k, n), n == k, a share size that is no multiple of 16, a misaligned pointer:
    // such a segment on its own, padded and encoded with its own stripe count
    for (size_t g : own) {
        if (data_len)
            if (int rc = ec_pad_segments(segs[g], 1, 0, data_len[g], (size_t)stripe, stream)) return rc;
        if (int rc = encode_range(c, segs[g], 1, nstripes[g], 0, nstripes[g], pieces[g], flags, s, false, true))
            return rc;
    }
    std::vector<int64_t> blocks(fast.size());
    for (size_t i = 0; i < fast.size(); i++) blocks[i] = fast[i].blocks;
    for (const sized::Pass &p : sized::split_passes(blocks.data(), fast.size(), sized::kPassSegs, sized::kPassTiles))
        if (int rc = encode_sized_pass(c, *ek, fast.data() + p.i0, p.i1 - p.i0, parity_only, s)) return rc;
    return EC_OK;
}

}  // extern "C"
