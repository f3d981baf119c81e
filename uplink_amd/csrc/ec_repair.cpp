// C-ABI, segment repair (include/uplink_ec.h ec_repair_segments_sets,
// ec_repair_segments_sized): the lost pieces of a batch of segments, each from
// its own share set -- and, in the sized call, of its own size -- regenerated
// straight from the k basis shares in one stream-ordered pass (rs_repair.hpp).
// The host chooses the basis as Rebuild does, solves each segment's rows in
// closed form (LagrangeBasis) and stages them; nothing waits for the stream.
#include "ec_internal.hpp"
#include "sized_geom.hpp"

namespace uplink_ec {
namespace capi {
namespace {

// One segment of a repair call as the host prepares it.
struct RepairSeg {
    std::vector<const uint8_t *> in;  // the k basis shares (infectious' choice, by position), then -- check -- the others
    std::vector<int> num;             // their piece numbers
    std::vector<int> tnum;            // targets
    std::vector<uint8_t *> out;
    size_t g = 0;                     // segment of the call
    int64_t nstripes = 0, chunks = 0, tiles = 0;  // the sized call: the segment's own geometry
    int rows = 0, nw = 2;
    bool bits = true;
};

// Segment `sg` of a call from its share list (ns numbers and pointers) and its
// target list (nt > 0 numbers and outputs), validated: the basis is infectious
// Rebuild's choice, then -- check -- the other shares by number.
int prepare_segment(const ec_ctx *c, bool check, int ns, const int *snum, const uint8_t *const *sp, int nt,
                    const int *tnum, uint8_t *const *op, RepairSeg &sg) {
    const int k = c->k, n = c->n, ess = c->ess;
    if (ns < k) return EC_ERR_NOT_ENOUGH_SHARES;
    bool given[256] = {}, wanted[256] = {};
    for (int i = 0; i < ns; i++) {
        if (snum[i] < 0 || snum[i] >= n) return EC_ERR_INVALID_SHARE;
        if (!sp[i]) return EC_ERR_INVALID_ARG;
        given[snum[i]] = true;
    }
    if (check && ns > kMaxOps) return EC_ERR_UNSUPPORTED;
    for (int r = 0; r < nt; r++) {
        if (tnum[r] < 0 || tnum[r] >= n) return EC_ERR_INVALID_SHARE;
        if (given[tnum[r]] || wanted[tnum[r]] || !op[r]) return EC_ERR_INVALID_ARG;
        wanted[tnum[r]] = true;
    }
    std::vector<int> order, ids;
    if (int rc = choose_shares(c, ns, snum, order, ids)) return rc;
    bool seen[256] = {};
    std::vector<char> chosen(ns, 0);
    for (int i = 0; i < k; i++) {
        if (seen[ids[i]]) return EC_ERR_SINGULAR;
        seen[ids[i]] = true;
        chosen[order[i]] = 1;
        sg.in.push_back(sp[order[i]]);
        sg.num.push_back(ids[i]);
    }
    if (check) {  // the other shares, by number (as the share-set decode orders them)
        std::vector<int> rest;
        for (int i = 0; i < ns; i++)
            if (!chosen[i]) rest.push_back(i);
        std::stable_sort(rest.begin(), rest.end(), [&](int x, int y) { return snum[x] < snum[y]; });
        for (int i : rest) {
            sg.in.push_back(sp[i]);
            sg.num.push_back(snum[i]);
        }
    }
    sg.tnum.assign(tnum, tnum + nt);
    sg.out.assign(op, op + nt);
    sg.rows = nt + (int)sg.in.size() - k;
    sg.nw = repair_waves(sg.rows);
    sg.bits = ess % 16 == 0;
    for (const uint8_t *p : sg.in) sg.bits = sg.bits && aligned16(p);
    for (const uint8_t *p : sg.out) sg.bits = sg.bits && aligned16(p);
    return EC_OK;
}

// A segment the bit-sliced kernel cannot take, through the plan path: the
// matrix from the host under a key of its own kind, the byte kernel with
// piece -> piece geometry (both strides ess, so a column's offset is the same
// in every share and output).
int repair_bytes(ec_ctx *c, const RepairSeg &sg, int64_t nstripes, int32_t *status, hipStream_t s) {
    const int k = c->k, nt = (int)sg.tnum.size();
    std::vector<int> key{-5};
    key.insert(key.end(), sg.num.begin(), sg.num.begin() + k);
    key.push_back(-6);
    key.insert(key.end(), sg.tnum.begin(), sg.tnum.end());
    key.push_back(-7);
    key.insert(key.end(), sg.num.begin() + k, sg.num.end());
    // every row from the k basis shares: the targets, then the other shares as predicted
    const LagrangeBasis L(sg.num.data(), k);
    std::vector<uint8_t> M((size_t)sg.rows * k);
    for (int r = 0; r < sg.rows; r++) L.row(gf_point(r < nt ? sg.tnum[r] : sg.num[k + r - nt]), &M[(size_t)r * k]);
    PlanPtr plan;
    if (int rc = matrix_plan(c, key, M.data(), sg.rows, k, &plan)) return rc;
    RsArgs a{};
    const uint8_t *base = sg.in[0];
    for (int j = 0; j < k; j++) base = std::min(base, sg.in[j]);
    a.in_base = base;
    a.in_stripe_stride = a.out_stripe_stride = c->ess;
    fill_geometry(a, c->ess, nstripes, 1);
    a.total_tiles = 1;  // byte kernel: total_tiles carries the segment count
    a.nin = k;
    a.coef_ld = plan->coef_ld;
    for (int j = 0; j < k; j++) {
        a.in_off[j] = sg.in[j] - base;
        a.copy_off[j] = -1;
    }
    for (int done = 0; done < sg.rows;) {
        const bool check = done >= nt;
        const int rows = std::min(kMaxOps, (check ? sg.rows : nt) - done);
        a.coef = plan->d_coef + done;
        a.nout = rows;
        if (check) {
            a.out_base = const_cast<uint8_t *>(base);  // (read only: the shares compared with)
            for (int r = 0; r < rows; r++) a.out_off[r] = sg.in[k + done - nt + r] - base;
            a.zero_check = (uint32_t *)status;
            HIP_TRY(launch_repair_check_bytes(a, s));
        } else {
            a.out_base = sg.out[done];
            for (int r = 0; r < rows; r++) a.out_off[r] = sg.out[done + r] - a.out_base;
            HIP_TRY(launch_matmul_bytes(a, s));
        }
        plan->note_use(s);
        plan->launches++;
        done += rows;
    }
    return EC_OK;
}

int repair_call(ec_ctx *c, std::vector<RepairSeg> &segs, int64_t nstripes, int32_t *dev_status, bool check,
                hipStream_t s) {
    const int k = c->k, ess = c->ess;
    const int64_t piece_len = nstripes * ess;
    std::vector<int> idx;  // the bit-sliced kernel's segments, by wave-count class
    for (size_t i = 0; i < segs.size(); i++)
        if (segs[i].bits) idx.push_back((int)i);
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return segs[x].nw < segs[y].nw; });
    const size_t nb = idx.size();
    for (auto &sg : segs)
        if (!sg.bits)
            if (int rc = repair_bytes(c, sg, nstripes, check ? dev_status + sg.g : nullptr, s)) return rc;
    if (nb == 0) return EC_OK;
    std::vector<size_t> eoff(nb + 1, 0);
    for (size_t q = 0; q < nb; q++) {
        const RepairSeg &sg = segs[idx[q]];
        eoff[q + 1] = eoff[q] + staged_entries((int)sg.in.size(), sg.rows, sg.nw);
    }
    const size_t h_stage = nb * sizeof(RepairStage), d_desc = up(nb * sizeof(RepairDesc), 256);
    StageBlock *b = block_acquire(c->repair, h_stage + eoff[nb], d_desc + eoff[nb] * 8);
    if (!b) return EC_ERR_DEVICE;
    RepairStage *stage = (RepairStage *)b->h;
    uint8_t *h_coef = b->h + h_stage;
    RepairDesc *d_descs = (RepairDesc *)b->d;
    uint64_t *d_tgt = (uint64_t *)(b->d + d_desc);
    std::vector<uint8_t> M;
    for (size_t q = 0; q < nb; q++) {
        const RepairSeg &sg = segs[idx[q]];
        const int nin = (int)sg.in.size(), nt = (int)sg.tnum.size(), nw = sg.nw;
        RepairStage &st = stage[q];
        memset(&st, 0, sizeof(st));
        for (int j = 0; j < nin; j++) st.d.in[j] = sg.in[j];
        for (int r = 0; r < nt; r++) st.d.out[r] = sg.out[r];
        st.d.tgt = d_tgt + eoff[q];
        st.d.status = check ? dev_status + sg.g : nullptr;
        st.d.nin = nin;
        st.d.nout = sg.rows;
        st.d.nstore = nt;
        st.d.nw = nw;
        st.coef = h_coef + eoff[q];
        st.entries = (int64_t)(eoff[q + 1] - eoff[q]);
        // the rows (targets, then the syndrome rows) in the leaf table's order
        M.resize((size_t)sg.rows * nin);
        solve_rows(sg.num.data(), k, nin, sg.tnum.data(), nt, M.data());
        pack_rows(M.data(), sg.rows, nin, nw, h_coef + eoff[q]);
    }
    hipError_t e = launch_repair_prep(stage, d_descs, (int)nb, c->jt_base, s);
    if (e != hipSuccess) {  // nothing was queued
        block_release(c->repair, b, false, s);
        return hip_fail(e);
    }
    const int64_t chunks = piece_len / 16, tiles = (chunks + kTileChunksHost - 1) / kTileChunksHost;
    for (size_t q0 = 0; q0 < nb && e == hipSuccess;) {
        const int nw = segs[idx[q0]].nw;
        size_t q1 = q0;
        // (more tiles than one launch takes: in parts)
        while (q1 < nb && segs[idx[q1]].nw == nw && (int64_t)(q1 + 1 - q0) * tiles <= share_max_tiles(nw)) q1++;
        RepairArgs a{};
        a.desc = d_descs + q0;
        a.piece_len = piece_len;
        a.chunks_per_seg = chunks;
        a.tiles_per_seg = tiles;
        a.total_tiles = tiles * (int64_t)(q1 - q0);
        a.chk_flag = c->d_chk;
        e = launch_repair(a, nw, s);
        q0 = q1;
    }
    block_release(c->repair, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    c->last_body = EC_BODY_JUMP_TABLE;
    return after_launch(c->d_chk, s);
}

// One pass of a sized call over segs[0..n), segments of their own sizes:
// rs_repair_sized_prep, then the tile kernel per wave-count class (in parts where
// a class has more tiles than a launch takes), all on stream s; staged as
// repair_call stages, plus the classes' tile maps (sized_geom.hpp).
int repair_sized_pass(ec_ctx *c, RepairSeg *const *segs, size_t n, int32_t *dev_status, bool check, hipStream_t s) {
    const int k = c->k;
    std::vector<int> nw(n);
    std::vector<int64_t> tiles(n);
    for (size_t i = 0; i < n; i++) {
        nw[i] = segs[i]->nw;
        tiles[i] = segs[i]->tiles;
    }
    const sized::Layout L = sized::layout(nw.data(), tiles.data(), n, share_max_tiles);
    std::vector<size_t> eoff(n + 1, 0);
    for (size_t q = 0; q < n; q++) {
        const RepairSeg &sg = *segs[L.idx[q]];
        eoff[q + 1] = eoff[q] + staged_entries((int)sg.in.size(), sg.rows, sg.nw);
    }
    const size_t h_stage = up(n * sizeof(RepairSizedStage), 16);
    const size_t d_desc = up(n * sizeof(RepairSizedDesc), 256), d_tgt_len = eoff[n] * 8;
    StageBlock *b = block_acquire(c->repair, h_stage + eoff[n], d_desc + d_tgt_len + (size_t)L.map_entries * 4);
    if (!b) return EC_ERR_DEVICE;
    RepairSizedStage *stage = (RepairSizedStage *)b->h;
    uint8_t *h_coef = b->h + h_stage;
    RepairSizedDesc *d_descs = (RepairSizedDesc *)b->d;
    uint64_t *d_tgt = (uint64_t *)(b->d + d_desc);
    uint32_t *d_map = (uint32_t *)(b->d + d_desc + d_tgt_len);
    std::vector<uint8_t> M;
    for (size_t q = 0; q < n; q++) {
        const RepairSeg &sg = *segs[L.idx[q]];
        const int nin = (int)sg.in.size(), nt = (int)sg.tnum.size();
        RepairSizedStage &st = stage[q];
        memset(&st, 0, sizeof(st));
        for (int j = 0; j < nin; j++) st.d.in[j] = sg.in[j];
        for (int r = 0; r < nt; r++) st.d.out[r] = sg.out[r];
        st.d.tgt = d_tgt + eoff[q];
        st.d.status = check ? dev_status + sg.g : nullptr;
        st.d.nin = nin;
        st.d.nout = sg.rows;
        st.d.nstore = nt;
        st.d.nw = sg.nw;
        st.d.chunks = sg.chunks;
        st.d.piece_len = sg.chunks * 16;
        st.d.tile0 = L.tile0[q];
        st.coef = h_coef + eoff[q];
        st.entries = (int64_t)(eoff[q + 1] - eoff[q]);
        st.map = d_map + L.map_off[q] + L.tile0[q];
        st.ntiles = sg.tiles;
        // the rows (targets, then the syndrome rows) in the leaf table's order
        M.resize((size_t)sg.rows * nin);
        solve_rows(sg.num.data(), k, nin, sg.tnum.data(), nt, M.data());
        pack_rows(M.data(), sg.rows, nin, sg.nw, h_coef + eoff[q]);
    }
    hipError_t e = launch_repair_sized_prep(stage, d_descs, (int)n, c->jt_base, s);
    if (e != hipSuccess) {  // nothing was queued
        block_release(c->repair, b, false, s);
        return hip_fail(e);
    }
    for (const sized::Launch &ln : L.launches) {
        RepairSizedArgs a{};
        a.desc = d_descs;
        a.map = d_map + ln.map_off;
        a.tile_base = ln.tile_base;
        a.total_tiles = ln.tiles;
        a.chk_flag = c->d_chk;
        e = launch_repair_sized(a, ln.nw, s);
        if (e != hipSuccess) break;
    }
    block_release(c->repair, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    c->last_body = EC_BODY_JUMP_TABLE;
    return after_launch(c->d_chk, s);
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_repair_segments_sets(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                            const uint8_t *const *pieces, const int *ntargets, const int *targets,
                            uint8_t *const *outs, size_t nstripes, int flags, int32_t *dev_status, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nshares || !nums || !pieces || !ntargets || !targets || !outs))) return EC_ERR_INVALID_ARG;
    if (flags & ~EC_FLAG_CHECK_SHARES) return EC_ERR_INVALID_ARG;
    const bool check = (flags & EC_FLAG_CHECK_SHARES) != 0;
    if (check && !dev_status) return EC_ERR_INVALID_ARG;
    if (nseg == 0 || nstripes == 0) return EC_OK;
    const int k = c->k, ess = c->ess;
    if (k > kMaxOps) return EC_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // every segment is validated before anything is queued
    std::vector<RepairSeg> segs;
    size_t soff = 0, toff = 0;
    for (size_t g = 0; g < nseg; g++) {
        const int ns = nshares[g], nt = ntargets[g];
        if (nt < 0) return EC_ERR_INVALID_ARG;
        const int *snum = nums + soff, *tnum = targets + toff;
        const uint8_t *const *sp = pieces + soff;
        uint8_t *const *op = outs + toff;
        soff += (size_t)std::max(ns, 0);
        toff += (size_t)nt;
        if (nt == 0) continue;
        RepairSeg sg;
        if (int rc = prepare_segment(c, check, ns, snum, sp, nt, tnum, op, sg)) return rc;
        sg.g = g;
        if (sg.bits) {
            const int64_t tiles = ((int64_t)nstripes * (ess / 16) + kTileChunksHost - 1) / kTileChunksHost;
            if (tiles > share_max_tiles(sg.nw)) return EC_ERR_UNSUPPORTED;
        }
        segs.push_back(std::move(sg));
    }
    DeviceGuard dg(c->device);
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    if (check) HIP_TRY(hipMemsetAsync(dev_status, 0, sizeof(int32_t) * nseg, s));
    if (segs.empty()) return EC_OK;
    return repair_call(c, segs, (int64_t)nstripes, dev_status, check, s);
}

int ec_repair_segments_sized(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                             const uint8_t *const *pieces, const int *ntargets, const int *targets,
                             uint8_t *const *outs, const size_t *nstripes, int flags, int32_t *dev_status,
                             ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nshares || !nums || !pieces || !ntargets || !targets || !outs || !nstripes)))
        return EC_ERR_INVALID_ARG;
    if (flags & ~EC_FLAG_CHECK_SHARES) return EC_ERR_INVALID_ARG;
    const bool check = (flags & EC_FLAG_CHECK_SHARES) != 0;
    if (check && !dev_status) return EC_ERR_INVALID_ARG;
    if (nseg == 0) return EC_OK;
    const int ess = c->ess;
    if (c->k > kMaxOps) return EC_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // every segment is validated before anything is queued
    std::vector<RepairSeg> segs;
    size_t soff = 0, toff = 0;
    for (size_t g = 0; g < nseg; g++) {
        const int ns = nshares[g], nt = ntargets[g];
        if (nt < 0) return EC_ERR_INVALID_ARG;
        const int *snum = nums + soff, *tnum = targets + toff;
        const uint8_t *const *sp = pieces + soff;
        uint8_t *const *op = outs + toff;
        soff += (size_t)std::max(ns, 0);
        toff += (size_t)nt;
        if (nt == 0 || nstripes[g] == 0) continue;
        RepairSeg sg;
        if (int rc = prepare_segment(c, check, ns, snum, sp, nt, tnum, op, sg)) return rc;
        sg.g = g;
        sg.chunks = sized::chunks_of(nstripes[g], ess);
        if (sg.chunks < 0) return EC_ERR_UNSUPPORTED;
        sg.nstripes = (int64_t)nstripes[g];
        sg.tiles = sized::tiles_of(sg.chunks);
        segs.push_back(std::move(sg));
    }
    DeviceGuard dg(c->device);
    // staging blocks are recycled by events behind launches that run: not under stream capture
    if (stream_is_capturing(s)) return EC_ERR_UNSUPPORTED;
    if (check) HIP_TRY(hipMemsetAsync(dev_status, 0, sizeof(int32_t) * nseg, s));
    // what the bit-sliced kernel cannot take: such a segment on its own, with its own stripe count
    std::vector<RepairSeg *> list;
    for (RepairSeg &sg : segs) {
        if (sg.bits) {
            list.push_back(&sg);
            continue;
        }
        if (int rc = repair_bytes(c, sg, sg.nstripes, check ? dev_status + sg.g : nullptr, s)) return rc;
    }
    std::vector<int64_t> tiles(list.size());
    for (size_t i = 0; i < list.size(); i++) tiles[i] = list[i]->tiles;
    for (const sized::Pass &p : sized::split_passes(tiles.data(), list.size(), sized::kPassSegs, sized::kPassTiles))
        if (int rc = repair_sized_pass(c, list.data() + p.i0, p.i1 - p.i0, dev_status, check, s)) return rc;
    return EC_OK;
}

}  // extern "C"
