// C-ABI, AES-256-GCM of many one-shot messages, a raw key each
// (include/uplink_ec.h ec_gcm_seal_messages / ec_gcm_open_messages): what the
// stream layer does through encryption.Encrypt / Decrypt / EncryptKey /
// DecryptKey -- aesgcm.Seal(nil, nonce[:12], data, nil) around every inline
// segment (splitter/splitter.go:189, streams/store.go:360-375), every content
// key (splitter.go:160, store.go:349) and the object's metadata -- for a list of
// messages, each with its own 32 key bytes, nonce, length and addresses, in one
// stream-ordered pass.  The kernel derives everything from the key bytes
// (aesgcm.hip gcm_messages), so the host only validates the list and stages one
// descriptor per message, in passes of gcmmsg::kPassMessages, in event-recycled
// blocks; nothing on the call path waits for the stream.
#include "aesgcm.hpp"
#include "ec_internal.hpp"
#include "gcm_msg_geom.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One pass over messages [i0, i1) of the call: gcm_msg_prep, then the cipher, on stream s.
int gcm_msg_pass(ec_ctx *c, size_t i0, size_t i1, size_t nmsg, const uint8_t *const *in, const size_t *len,
                 const uint8_t *keys, const uint8_t *nonces, uint8_t *const *out, int32_t *status, bool open,
                 hipStream_t s) {
    const size_t n = i1 - i0, bytes = n * sizeof(GcmMsgDesc);
    StageBlock *b = block_acquire(c->gcm_sized, bytes, up(bytes, 256));
    if (!b) return EC_ERR_DEVICE;
    GcmMsgDesc *stage = (GcmMsgDesc *)b->h;
    for (size_t q = 0; q < n; q++) {
        GcmMsgDesc &d = stage[q];
        d.in = in[i0 + q];
        d.out = out[i0 + q];
        d.len = (uint32_t)len[i0 + q];
        d.msg = (uint32_t)(i0 + q);
    }
    const GcmMsgPass p{stage, (GcmMsgDesc *)b->d, (uint32_t)n, keys, nonces, status, (uint32_t)nmsg, c->d_chk};
    const hipError_t e = gcm_launch_messages(p, open, s);
    // (a failed launch may have queued the prep launch before it: the block waits for the stream)
    block_release(c->gcm_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    (open ? c->gm_open : c->gm_seal).fetch_add(1, std::memory_order_relaxed);
    c->gm_passes.fetch_add(1, std::memory_order_relaxed);
    return after_launch(c->d_chk, s);
}

int gcm_msg_run(const ec_ctx *cc, size_t nmsg, const uint8_t *const *in, const size_t *len, const uint8_t *keys,
                const uint8_t *nonces, uint8_t *const *out, int32_t *status, bool open, hipStream_t s) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c) return EC_ERR_INVALID_ARG;
    if (nmsg == 0) return EC_OK;
    if (!in || !len || !out || !keys || !nonces || (open && !status)) return EC_ERR_INVALID_ARG;
    if (nmsg > 0xFFFFFFFFu) return EC_ERR_UNSUPPORTED;
    // every message is validated before anything is queued
    for (size_t i = 0; i < nmsg; i++) {
        if (len[i] > gcmmsg::kMaxLen) return EC_ERR_UNSUPPORTED;
        // the sealed side always holds the tag; the plaintext side of an empty message holds nothing
        const bool need_in = open || len[i] > 0, need_out = !open || len[i] > 0;
        if ((need_in && !in[i]) || (need_out && !out[i])) return EC_ERR_INVALID_ARG;
    }
    DeviceGuard dg(c->device);
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    for (const sized::Pass &p : gcmmsg::split(nmsg))
        if (int rc = gcm_msg_pass(c, p.i0, p.i1, nmsg, in, len, keys, nonces, out, status, open, s)) return rc;
    return EC_OK;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_gcm_seal_messages(const ec_ctx *ctx, size_t nmsg, const uint8_t *const *plain, const size_t *len,
                         const uint8_t *dev_keys32, const uint8_t *dev_nonces, uint8_t *const *out, ec_stream stream) {
    return gcm_msg_run(ctx, nmsg, plain, len, dev_keys32, dev_nonces, out, nullptr, false, (hipStream_t)stream);
}

int ec_gcm_open_messages(const ec_ctx *ctx, size_t nmsg, const uint8_t *const *cipher, const size_t *len,
                         const uint8_t *dev_keys32, const uint8_t *dev_nonces, uint8_t *const *out,
                         int32_t *dev_status, ec_stream stream) {
    return gcm_msg_run(ctx, nmsg, cipher, len, dev_keys32, dev_nonces, out, dev_status, true, (hipStream_t)stream);
}

int ec_gcm_messages_stats(const ec_ctx *c, unsigned long long *seal_launches, unsigned long long *open_launches,
                          unsigned long long *passes, unsigned long long *pass_messages) {
    if (!c) return EC_ERR_INVALID_ARG;
    if (seal_launches) *seal_launches = c->gm_seal.load(std::memory_order_relaxed);
    if (open_launches) *open_launches = c->gm_open.load(std::memory_order_relaxed);
    if (passes) *passes = c->gm_passes.load(std::memory_order_relaxed);
    if (pass_messages) *pass_messages = gcmmsg::kPassMessages;
    return EC_OK;
}

}  // extern "C"
