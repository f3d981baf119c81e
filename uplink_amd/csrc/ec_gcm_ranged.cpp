// C-ABI, AES-256-GCM open of byte ranges of many segments at once
// (include/uplink_ec.h ec_gcm_open_ranges_sized): what a ranged download does
// through decryptRanger's Range (streams/store.go:347-382, encryption.Transform)
// -- the cipher blocks that cover the range opened under nonce + their absolute
// number, the head of the first discarded, the length limited -- for a batch of
// ranges, each of its own segment, key and nonce, in one stream-ordered pass.
// The host validates every segment (range_geom.hpp), lays each pass out as the
// sized cipher does (gcm_sized_geom.hpp) and stages one descriptor per segment
// in event-recycled blocks; nothing on the call path waits for the stream.
#include "aesgcm.hpp"
#include "ec_internal.hpp"
#include "gcm_sized_geom.hpp"
#include "range_geom.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One segment the ranged kernel takes (skipped segments are not listed).
struct GcmRange {
    const uint8_t *in;
    uint8_t *out;
    uint64_t length;
    uint32_t head, nblocks, first_block, seg;
};

// One pass over segs[0..n): gcm_ranged_prep, then the cipher, on stream s.
int gcm_ranged_pass(ec_ctx *c, const GcmRange *segs, size_t n, size_t nseg, size_t in_block, const void *keys,
                    const uint8_t *nonces, int32_t *status, hipStream_t s) {
    std::vector<uint64_t> nb(n);
    for (size_t i = 0; i < n; i++) nb[i] = segs[i].nblocks;
    const gcmsized::Layout L = gcmsized::layout(nb.data(), n, gcm_target_grid());
    if (L.map.empty()) return EC_OK;
    const size_t d_desc = up(n * sizeof(GcmRangedDesc), 256);
    StageBlock *b = block_acquire(c->gcm_sized, n * sizeof(GcmRangedDesc), d_desc + up(L.map.size() * 4, 256));
    if (!b) return EC_ERR_DEVICE;
    GcmRangedDesc *stage = (GcmRangedDesc *)b->h;
    bool mixed = false;
    for (size_t i = 0; i < n; i++) {
        GcmRangedDesc &d = stage[i];
        d.in = segs[i].in;
        d.out = segs[i].out;
        d.length = segs[i].length;
        d.head = segs[i].head;
        d.nblocks = segs[i].nblocks;
        d.first_block = segs[i].first_block;
        d.wg0 = L.wg0[i];
        d.wgs = L.wgs[i];
        d.seg = segs[i].seg;
        // output slot s of block r lies at out + r*in_block + 16s - head, source slots at in + r*(in_block+16) + 16s
        const bool aligned = aligned16(d.in) && aligned16(d.out) && d.head % 16 == 0;
        d.flags = aligned ? 0 : kGcmRangedBytewise;
        d.rsv = 0;
        mixed |= !aligned;
    }
    GcmRangedPass p{};
    p.stage = stage;
    p.desc = (GcmRangedDesc *)b->d;
    p.map = (uint32_t *)(b->d + d_desc);
    p.n = (uint32_t)n;
    p.wgs = (uint32_t)L.map.size();
    p.sched = static_cast<const GcmSched *>(keys);
    p.nonces = nonces;
    p.status = status;
    p.nseg = (uint32_t)nseg;
    p.in_block = (uint32_t)in_block;
    p.chk_flag = c->d_chk;
    p.mixed = mixed;
    const hipError_t e = gcm_launch_ranged(p, s);
    // (a failed launch may have queued the prep launch before it: the block waits for the stream)
    block_release(c->gcm_sized, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    c->gr_open.fetch_add(1, std::memory_order_relaxed);
    c->gr_passes.fetch_add(1, std::memory_order_relaxed);
    return after_launch(c->d_chk, s);
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_gcm_open_ranges_sized(const ec_ctx *cc, size_t nseg, const uint8_t *const *cipher, const size_t *first_block,
                             const size_t *nblocks, const size_t *head, const size_t *length, size_t in_block,
                             const void *dev_keys, const uint8_t *dev_nonces, uint8_t *const *out, int32_t *dev_status,
                             ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    hipStream_t s = (hipStream_t)stream;
    if (!c) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    if (!cipher || !first_block || !nblocks || !head || !length || !out || !dev_keys || !dev_nonces || !dev_status)
        return EC_ERR_INVALID_ARG;
    if (in_block == 0 || in_block > (1u << 24) || in_block % 16 || nseg > 0xFFFFFFFFu) return EC_ERR_UNSUPPORTED;
    // every segment is validated before anything is queued
    std::vector<GcmRange> list;
    list.reserve(nseg);
    for (size_t g = 0; g < nseg; g++) {
        if (!rangegeom::covers(head[g], length[g], in_block, nblocks[g])) return EC_ERR_INVALID_ARG;
        if (first_block[g] > rangegeom::kMaxBlockEnd || nblocks[g] > rangegeom::kMaxBlockEnd - first_block[g])
            return EC_ERR_UNSUPPORTED;
        if (nblocks[g] == 0) continue;  // (its length is 0)
        if (!cipher[g] || !out[g]) return EC_ERR_INVALID_ARG;
        list.push_back({cipher[g], out[g], (uint64_t)length[g], (uint32_t)head[g], (uint32_t)nblocks[g],
                        (uint32_t)first_block[g], (uint32_t)g});
    }
    DeviceGuard dg(c->device);
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    // the status words: set once before the first pass, finished once after the last
    HIP_TRY(gcm_status_launch(dev_status, (uint32_t)nseg, false, s));
    for (const sized::Pass &p : gcmsized::split(list.size()))
        if (int rc = gcm_ranged_pass(c, list.data() + p.i0, p.i1 - p.i0, nseg, in_block, dev_keys, dev_nonces,
                                     dev_status, s))
            return rc;
    HIP_TRY(gcm_status_launch(dev_status, (uint32_t)nseg, true, s));
    return EC_OK;
}

int ec_gcm_ranged_stats(const ec_ctx *c, unsigned long long *open_launches, unsigned long long *passes) {
    if (!c) return EC_ERR_INVALID_ARG;
    if (open_launches) *open_launches = c->gr_open.load(std::memory_order_relaxed);
    if (passes) *passes = c->gr_passes.load(std::memory_order_relaxed);
    return EC_OK;
}

}  // extern "C"
