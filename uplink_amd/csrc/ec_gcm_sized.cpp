// C-ABI, AES-256-GCM with a size per segment (include/uplink_ec.h
// ec_gcm_seal_segments_sized, ec_gcm_open_segments_sized): what the upload's
// splitter does through TransformWriterPadded(NewEncrypter(...))
// (splitter/splitter.go:156,170) and the download through decryptRanger
// (streams/store.go:347-382), for a batch of segments of as many sizes as
// objects, each under its own key and nonce, in one stream-ordered pass.  The
// host validates every segment, lays each pass out (gcm_sized_geom.hpp) and
// stages one record per segment in event-recycled blocks, as the sized hash does
// (ec_hash_sized.cpp); nothing on the call path waits for the stream.
#include "aesgcm.hpp"
#include "ec_internal.hpp"
#include "gcm_sized_geom.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One segment the sized kernel takes (skipped segments are not listed).
struct GcmSeg {
    const uint8_t *in;
    uint8_t *out;
    uint32_t nblocks, seg;
    uint64_t data_len;
    uint32_t pad;  // 0: already padded
};

// One pass over segs[0..n): gcm_sized_prep, then the cipher, on stream s.
int gcm_sized_pass(ec_ctx *c, const GcmSeg *segs, size_t n, size_t nseg, size_t in_block, const void *keys,
                   const uint8_t *nonces, int32_t *status, bool open, hipStream_t s) {
    std::vector<uint64_t> nb(n);
    for (size_t i = 0; i < n; i++) nb[i] = segs[i].nblocks;
    const gcmsized::Layout L = gcmsized::layout(nb.data(), n, gcm_target_grid());
    if (L.map.empty()) return EC_OK;
    const size_t d_desc = up(n * sizeof(GcmSizedDesc), 256);
    StageBlock *b = block_acquire(c->gcm_sized, n * sizeof(GcmSizedStage), d_desc + up(L.map.size() * 4, 256));
    if (!b) return EC_ERR_DEVICE;
    GcmSizedStage *stage = (GcmSizedStage *)b->h;
    for (size_t i = 0; i < n; i++) {
        GcmSizedStage &st = stage[i];
        st.d.in = segs[i].in;
        st.d.out = segs[i].out;
        st.d.nblocks = segs[i].nblocks;
        st.d.wg0 = L.wg0[i];
        st.d.wgs = L.wgs[i];
        st.d.seg = segs[i].seg;
        st.data_len = segs[i].data_len;
        st.pad = segs[i].pad;
        st.rsv = 0;
    }
    GcmSizedPass p{};
    p.stage = stage;
    p.desc = (GcmSizedDesc *)b->d;
    p.map = (uint32_t *)(b->d + d_desc);
    p.n = (uint32_t)n;
    p.wgs = (uint32_t)L.map.size();
    p.sched = static_cast<const GcmSched *>(keys);
    p.nonces = nonces;
    p.status = status;
    p.nseg = (uint32_t)nseg;
    p.in_block = (uint32_t)in_block;
    p.chk_flag = c->d_chk;
    const hipError_t e = gcm_launch_sized(p, open, s);
    // (a failed launch may have queued the prep launch before it: the block waits for the stream)
    block_release(c->gcm_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    (open ? c->gs_open : c->gs_seal).fetch_add(1, std::memory_order_relaxed);
    c->gs_passes.fetch_add(1, std::memory_order_relaxed);
    return after_launch(c->d_chk, s);
}

int gcm_sized(const ec_ctx *cc, size_t nseg, const uint8_t *const *in, const size_t *nblocks, const size_t *data_len,
              size_t in_block, const void *keys, const uint8_t *nonces, uint8_t *const *out, int32_t *status, bool open,
              hipStream_t s) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    if (!in || !nblocks || !out || !keys || !nonces || (open && !status)) return EC_ERR_INVALID_ARG;
    if (in_block == 0 || in_block > (1u << 24) || in_block % 16 || nseg > 0xFFFFFFFFu) return EC_ERR_UNSUPPORTED;
    // every segment is validated before anything is queued
    std::vector<GcmSeg> list;
    list.reserve(nseg);
    for (size_t g = 0; g < nseg; g++) {
        if (nblocks[g] == 0) continue;
        if (!in[g] || !out[g]) return EC_ERR_INVALID_ARG;
        if (nblocks[g] > gcmsized::kMaxBlocks || !aligned16(in[g]) || !aligned16(out[g])) return EC_ERR_UNSUPPORTED;
        uint32_t pad = 0;
        if (data_len) {
            if (!gcmsized::pad_matches(data_len[g], nblocks[g], in_block)) return EC_ERR_INVALID_ARG;
            pad = (uint32_t)gcmsized::pad_amount(data_len[g], in_block);
        }
        list.push_back({in[g], out[g], (uint32_t)nblocks[g], (uint32_t)g, data_len ? (uint64_t)data_len[g] : 0, pad});
    }
    DeviceGuard dg(c->device);
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    // the status words: set once before the first pass, finished once after the last
    if (open) HIP_TRY(gcm_status_launch(status, (uint32_t)nseg, false, s));
    for (const sized::Pass &p : gcmsized::split(list.size()))
        if (int rc = gcm_sized_pass(c, list.data() + p.i0, p.i1 - p.i0, nseg, in_block, keys, nonces, status, open, s))
            return rc;
    if (open) HIP_TRY(gcm_status_launch(status, (uint32_t)nseg, true, s));
    return EC_OK;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_gcm_seal_segments_sized(const ec_ctx *ctx, size_t nseg, uint8_t *const *plain, const size_t *nblocks,
                               const size_t *data_len, size_t in_block, const void *dev_keys,
                               const uint8_t *dev_nonces, uint8_t *const *out, ec_stream stream) {
    return gcm_sized(ctx, nseg, plain, nblocks, data_len, in_block, dev_keys, dev_nonces, out, nullptr, false,
                     (hipStream_t)stream);
}

int ec_gcm_open_segments_sized(const ec_ctx *ctx, size_t nseg, const uint8_t *const *cipher, const size_t *nblocks,
                               size_t in_block, const void *dev_keys, const uint8_t *dev_nonces,
                               uint8_t *const *out, int32_t *dev_status, ec_stream stream) {
    return gcm_sized(ctx, nseg, cipher, nblocks, nullptr, in_block, dev_keys, dev_nonces, out, dev_status, true,
                     (hipStream_t)stream);
}

int ec_gcm_sized_stats(const ec_ctx *c, unsigned long long *seal_launches, unsigned long long *open_launches,
                       unsigned long long *passes) {
    if (!c) return EC_ERR_INVALID_ARG;
    if (seal_launches) *seal_launches = c->gs_seal.load(std::memory_order_relaxed);
    if (open_launches) *open_launches = c->gs_open.load(std::memory_order_relaxed);
    if (passes) *passes = c->gs_passes.load(std::memory_order_relaxed);
    return EC_OK;
}

}  // extern "C"
