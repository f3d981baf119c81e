// C-ABI, share-set calls with a size per segment (include/uplink_ec.h
// ec_rebuild_segments_sized, ec_decode_segments_sized): a batch of downloads of
// as many sizes as objects, each rebuilt or decoded from its own share set, in
// one stream-ordered pass (rs_sized.hpp).  The host chooses the basis as
// Rebuild does, solves each segment's rows in closed form (LagrangeBasis) and
// stages them with the geometry (sized_geom.hpp) in event-recycled blocks, as
// segment repair does (ec_repair.cpp); nothing on the Rebuild path waits for
// the stream.
#include "ec_stage_pass.hpp"
#include "rs_sized.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One segment of a sized call as the host prepares it: the inputs in the
// kernel's order (infectious' k chosen shares by position, then -- Decode --
// the other shares by number) and the rows (missing data positions, then one
// syndrome row per non-basis input).
struct SizedSeg {
    std::vector<const uint8_t *> in;
    std::vector<int> num;
    std::vector<int> missing;
    uint8_t *out = nullptr;
    size_t g = 0;  // segment of the call
    int64_t nstripes = 0, chunks = 0, tiles = 0;
    int rows = 0, nw = 2;
    bool bits = true;  // the bit-sliced pass takes it
    bool own = false;  // Decode of more shares than a launch takes: ec_decode_segments on its own
};

// Fill `sg` from (nshares, nums, pieces).  Errors as Rebuild / Decode report
// them (an invalid share id, a repeated share chosen twice: singular).
int prepare_segment(const ec_ctx *c, int nshares, const int *nums, const uint8_t *const *pieces, bool decode,
                    SizedSeg &sg) {
    const int k = c->k;
    sg.own = decode && nshares > kMaxOps;
    const bool rest = decode && !sg.own;  // the other shares too, by number (as the share-set decode orders them)
    int pos[kMaxOps], nin, nst;
    sg.num.resize(rest ? nshares : k);
    sg.missing.resize(k);
    if (int rc = pick_inputs(k, c->n, nshares, nums, decode, rest, pos, sg.num.data(), sg.missing.data(), nin, nst))
        return rc;
    sg.missing.resize(nst);
    for (int j = 0; j < nin; j++) sg.in.push_back(pieces[pos[j]]);
    sg.rows = nst + nin - k;
    sg.nw = sets_waves(sg.rows);
    return EC_OK;
}

// One pass over segs[0..n): rs_sized_prep, then the tile kernel per wave-count
// class (in parts where a class has more tiles than a launch takes), all on
// stream s.  With `bad` (Decode), waits and returns per segment the count of
// syndrome failures.
int sized_pass(ec_ctx *c, SizedSeg *const *segs, size_t n, hipStream_t s, std::vector<uint32_t> *bad) {
    const int k = c->k, ess = c->ess;
    std::vector<int> nw(n);
    std::vector<int64_t> tiles(n);
    int widest = 2;
    for (size_t i = 0; i < n; i++) widest = std::max(widest, segs[i]->nw);
    for (size_t i = 0; i < n; i++) {
        if (c->sized_merge) segs[i]->nw = widest;  // (the A/B knob: one class, one launch)
        nw[i] = segs[i]->nw;
        tiles[i] = segs[i]->tiles;
    }
    const sized::Layout L = sized::layout(nw.data(), tiles.data(), n, share_max_tiles);
    using Pass = StagedPass<SizedStage>;
    return staged_pass<SizedStage>(
        c, c->sized, n, [&](size_t q) -> const SizedSeg & { return *segs[L.idx[q]]; }, &SizedSeg::missing, &L,
        bad ? n * 4 : 0,  // Decode: the segments' syndrome counters, and where they are read back to
        [&](SizedStage &st, const SizedSeg &sg, size_t q, const Pass &p) {
            for (int j = 0; j < st.d.nin; j++) st.d.copy_off[j] = j < k && sg.num[j] < k ? sg.num[j] * ess : -1;
            for (size_t r = 0; r < sg.missing.size(); r++) st.d.out_off[r] = sg.missing[r] * ess;
            st.d.out = sg.out;
            st.d.zero_check = bad ? (uint32_t *)p.d_extra + q : nullptr;
            st.d.spad = st.d.piece_len * k;
        },
        launch_sized_prep,
        [&](const Pass &p) {
            hipError_t e = hipSuccess;
            for (size_t i = 0; i < L.launches.size() && e == hipSuccess; i++) {
                const sized::Launch &ln = L.launches[i];
                SizedArgs a{};
                a.desc = p.desc;
                a.map = p.map + ln.map_off;
                a.tile_base = ln.tile_base;
                a.total_tiles = ln.tiles;
                a.ess = ess;
                a.cps = ess / 16;
                a.k = k;
                a.chk_flag = c->d_chk;
                e = launch_matmul_sized(a, ln.nw, s);
            }
            return e;
        },
        s,
        [&](const Pass &p) {
            if (!bad) return hipSuccess;
            // (the block stays this caller's until the counts are read: Decode returns when done)
            const uint32_t *h_cnt = (const uint32_t *)p.h_extra;
            hipError_t e = hipMemcpyAsync(p.h_extra, p.d_extra, n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            bad->assign(n, 0);
            for (size_t q = 0; q < n && e == hipSuccess; q++) (*bad)[L.idx[q]] = h_cnt[q];
            return e;
        });
}

int sized_call(ec_ctx *c, size_t nseg, const int *nshares, const int *nums, const uint8_t *const *pieces,
               const size_t *nstripes, uint8_t *const *outs, int *seg_rc, hipStream_t s, bool decode, bool *queued) {
    const int k = c->k, ess = c->ess;
    *queued = false;
    if (k > kMaxOps) return EC_ERR_UNSUPPORTED;
    // every segment is validated before anything is queued
    std::vector<size_t> off(nseg + 1, 0);
    for (size_t g = 0; g < nseg; g++) off[g + 1] = off[g] + (size_t)std::max(nshares[g], 0);
    std::vector<SizedSeg> segs;
    for (size_t g = 0; g < nseg; g++) {
        if (nstripes[g] == 0) continue;
        const int ns = nshares[g];
        if (ns < k) return EC_ERR_NOT_ENOUGH_SHARES;
        if (!outs[g]) return EC_ERR_INVALID_ARG;
        const uint8_t *const *sp = pieces + off[g];
        for (int i = 0; i < ns; i++)
            if (!sp[i]) return EC_ERR_INVALID_ARG;
        const int64_t chunks = sized::chunks_of(nstripes[g], ess);
        if (chunks < 0) return EC_ERR_UNSUPPORTED;
        segs.emplace_back();
        SizedSeg &sg = segs.back();
        if (int rc = prepare_segment(c, ns, nums + off[g], sp, decode, sg)) return rc;
        sg.g = g;
        sg.out = outs[g];
        sg.nstripes = (int64_t)nstripes[g];
        sg.chunks = chunks;
        sg.tiles = sized::tiles_of(chunks);
        sg.bits = !sg.own && ess % 16 == 0 && aligned16(outs[g]);
        for (int i = 0; i < ns; i++) sg.bits = sg.bits && aligned16(sp[i]);
    }
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    *queued = true;
    std::vector<int> rcs(nseg, EC_OK);
    // A segment's own outcome.  Too few shares is an argument error of the call, found above
    // before anything is queued (every segment here has at least k).  infectious words one
    // more case that way: an error detected where the surplus is too small to correct any
    // (fewer than k + 2 shares, Berlekamp-Welch's e = 0).  As a segment's outcome that is more
    // errors than its shares correct: EC_ERR_TOO_MANY_ERRORS.
    auto decode_own = [&](size_t g) {
        const int rc = ec_decode_segments(c, nshares[g], nums + off[g], (uint8_t *const *)pieces + off[g], nstripes[g],
                                          outs[g], (ec_stream)s);
        return rc == EC_ERR_NOT_ENOUGH_SHARES ? EC_ERR_TOO_MANY_ERRORS : rc;
    };
    // byte kernel / more inputs than a launch takes: such a segment on its own, with its own stripe count
    std::vector<SizedSeg *> list;
    for (SizedSeg &sg : segs) {
        if (sg.bits) {
            list.push_back(&sg);
            continue;
        }
        const size_t g = sg.g;
        if (decode) {
            rcs[g] = decode_own(g);
        } else if (int rc = rebuild_device(c, nshares[g], nums + off[g], pieces + off[g], ess, sg.nstripes, 1, 0, 0,
                                           outs[g], s)) {
            return rc;
        }
    }
    std::vector<int64_t> tiles(list.size());
    for (size_t i = 0; i < list.size(); i++) tiles[i] = list[i]->tiles;
    for (const sized::Pass &p : sized::split_passes(tiles.data(), list.size(), sized::kPassSegs, sized::kPassTiles)) {
        std::vector<uint32_t> bad;
        if (int rc = sized_pass(c, list.data() + p.i0, p.i1 - p.i0, s, decode ? &bad : nullptr)) return rc;
        // Decode: a segment whose syndromes are not all zero is corrected (in the caller's
        // pieces, as infectious corrects share.Data) and rebuilt on its own; its outcome is
        // its own, and the others go on
        for (size_t i = p.i0; i < p.i1 && decode; i++)
            if (bad[i - p.i0]) rcs[list[i]->g] = decode_own(list[i]->g);
    }
    int first = EC_OK;
    for (size_t g = 0; g < nseg; g++) {
        if (seg_rc) seg_rc[g] = rcs[g];
        if (first == EC_OK) first = rcs[g];
    }
    return first;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_rebuild_segments_sized(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                              const uint8_t *const *pieces, const size_t *nstripes, uint8_t *const *outs,
                              ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nshares || !nums || !pieces || !nstripes || !outs))) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    DeviceGuard dg(c->device);
    bool queued;
    return sized_call(c, nseg, nshares, nums, pieces, nstripes, outs, nullptr, (hipStream_t)stream, false, &queued);
}

int ec_decode_segments_sized(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                             uint8_t *const *pieces, const size_t *nstripes, uint8_t *const *outs, int *seg_rc,
                             ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nshares || !nums || !pieces || !nstripes || !outs))) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    DeviceGuard dg(c->device);
    bool queued;
    int rc = sized_call(c, nseg, nshares, nums, (const uint8_t *const *)pieces, nstripes, outs, seg_rc,
                        (hipStream_t)stream, true, &queued);
    // (nothing to wait for after an argument error, and no wait on a capturing stream)
    if (queued && hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == EC_OK) rc = EC_ERR_DEVICE;
    return rc;
}

}  // extern "C"
