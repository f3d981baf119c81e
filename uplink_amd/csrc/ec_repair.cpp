// C-ABI, segment repair (include/uplink_ec.h ec_repair_segments_sets,
// ec_repair_segments_sized): the lost pieces of a batch of segments, each from
// its own share set -- and, in the sized call, of its own size -- regenerated
// straight from the k basis shares in one stream-ordered pass (rs_repair.hpp).
// The host chooses the basis as Rebuild does, solves each segment's rows in
// closed form (LagrangeBasis) and stages them; nothing waits for the stream.
#include "ec_stage_pass.hpp"

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
    int64_t nstripes = 0, chunks = 0, tiles = 0;  // its geometry (the sized call: its own)
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
    int pos[kMaxOps], nin, nparity;
    sg.num.resize(check ? ns : k);
    if (int rc = pick_inputs(k, n, ns, snum, false, check, pos, sg.num.data(), nullptr, nin, nparity)) return rc;
    for (int j = 0; j < nin; j++) sg.in.push_back(sp[pos[j]]);
    sg.tnum.assign(tnum, tnum + nt);
    sg.out.assign(op, op + nt);
    sg.rows = nt + nin - k;
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

// The fields only a repair descriptor has (RepairDesc and RepairSizedDesc alike).
auto repair_fields(int32_t *dev_status, bool check) {
    return [=](auto &st, const RepairSeg &sg, size_t, const auto &) {
        for (size_t r = 0; r < sg.out.size(); r++) st.d.out[r] = sg.out[r];
        st.d.status = check ? dev_status + sg.g : nullptr;
        st.d.nw = sg.nw;
    };
}

// The pass of ec_repair_segments_sets over segs[0..n), all of one size:
// rs_repair_prep, then the tile kernel per wave-count class over whole segments
// (a class of more tiles than one launch takes in parts), all on stream s.
int repair_call(ec_ctx *c, RepairSeg **segs, size_t n, int32_t *dev_status, bool check, hipStream_t s) {
    std::stable_sort(segs, segs + n, [](const RepairSeg *x, const RepairSeg *y) { return x->nw < y->nw; });
    return staged_pass<RepairStage>(
        c, c->repair, n, [&](size_t q) -> const RepairSeg & { return *segs[q]; }, &RepairSeg::tnum, nullptr, 0,
        repair_fields(dev_status, check), launch_repair_prep,
        [&](const StagedPass<RepairStage> &p) {
            const int64_t chunks = segs[0]->chunks, tiles = segs[0]->tiles;
            hipError_t e = hipSuccess;
            for (size_t q0 = 0; q0 < n && e == hipSuccess;) {
                const int nw = segs[q0]->nw;
                size_t q1 = q0;
                // (more tiles than one launch takes: in parts)
                while (q1 < n && segs[q1]->nw == nw && (int64_t)(q1 + 1 - q0) * tiles <= share_max_tiles(nw)) q1++;
                RepairArgs a{};
                a.desc = p.desc + q0;
                a.piece_len = chunks * 16;
                a.chunks_per_seg = chunks;
                a.tiles_per_seg = tiles;
                a.total_tiles = tiles * (int64_t)(q1 - q0);
                a.chk_flag = c->d_chk;
                e = launch_repair(a, nw, s);
                q0 = q1;
            }
            return e;
        },
        s);
}

// One pass of a sized call over segs[0..n), segments of their own sizes:
// rs_repair_sized_prep, then the tile kernel per wave-count class (in parts where
// a class has more tiles than a launch takes), all on stream s; staged as
// repair_call stages, plus the classes' tile maps (sized_geom.hpp).
int repair_sized_pass(ec_ctx *c, RepairSeg *const *segs, size_t n, int32_t *dev_status, bool check, hipStream_t s) {
    std::vector<int> nw(n);
    std::vector<int64_t> tiles(n);
    for (size_t i = 0; i < n; i++) {
        nw[i] = segs[i]->nw;
        tiles[i] = segs[i]->tiles;
    }
    const sized::Layout L = sized::layout(nw.data(), tiles.data(), n, share_max_tiles);
    return staged_pass<RepairSizedStage>(
        c, c->repair, n, [&](size_t q) -> const RepairSeg & { return *segs[L.idx[q]]; }, &RepairSeg::tnum, &L, 0,
        repair_fields(dev_status, check), launch_repair_sized_prep,
        [&](const StagedPass<RepairSizedStage> &p) {
            hipError_t e = hipSuccess;
            for (size_t i = 0; i < L.launches.size() && e == hipSuccess; i++) {
                const sized::Launch &ln = L.launches[i];
                RepairSizedArgs a{};
                a.desc = p.desc;
                a.map = p.map + ln.map_off;
                a.tile_base = ln.tile_base;
                a.total_tiles = ln.tiles;
                a.chk_flag = c->d_chk;
                e = launch_repair_sized(a, ln.nw, s);
            }
            return e;
        },
        s);
}

// Both exports: segment g has nstripes_of[g] stripes, or -- nstripes_of null --
// every segment has `nstripes`.
int repair_export(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums, const uint8_t *const *pieces,
                  const int *ntargets, const int *targets, uint8_t *const *outs, const size_t *nstripes_of,
                  size_t nstripes, int flags, int32_t *dev_status, ec_stream stream) {
    ec_ctx *c = const_cast<ec_ctx *>(cc);
    if (!c || (nseg && (!nshares || !nums || !pieces || !ntargets || !targets || !outs))) return EC_ERR_INVALID_ARG;
    if (flags & ~EC_FLAG_CHECK_SHARES) return EC_ERR_INVALID_ARG;
    const bool check = (flags & EC_FLAG_CHECK_SHARES) != 0;
    if (check && !dev_status) return EC_ERR_INVALID_ARG;
    if (nseg == 0 || (!nstripes_of && nstripes == 0)) return EC_OK;
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
        const size_t stripes = nstripes_of ? nstripes_of[g] : nstripes;
        if (nt == 0 || stripes == 0) continue;
        RepairSeg sg;
        if (int rc = prepare_segment(c, check, ns, snum, sp, nt, tnum, op, sg)) return rc;
        sg.g = g;
        sg.nstripes = (int64_t)stripes;
        // (one size for all: only what the one launch per class cannot take is refused, below)
        sg.chunks = nstripes_of ? sized::chunks_of(stripes, ess) : sg.nstripes * (ess / 16);
        if (sg.chunks < 0) return EC_ERR_UNSUPPORTED;
        sg.tiles = sized::tiles_of(sg.chunks);
        if (!nstripes_of && sg.bits && sg.tiles > share_max_tiles(sg.nw)) return EC_ERR_UNSUPPORTED;
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
    if (!nstripes_of) return list.empty() ? EC_OK : repair_call(c, list.data(), list.size(), dev_status, check, s);
    std::vector<int64_t> tiles(list.size());
    for (size_t i = 0; i < list.size(); i++) tiles[i] = list[i]->tiles;
    for (const sized::Pass &p : sized::split_passes(tiles.data(), list.size(), sized::kPassSegs, sized::kPassTiles))
        if (int rc = repair_sized_pass(c, list.data() + p.i0, p.i1 - p.i0, dev_status, check, s)) return rc;
    return EC_OK;
}

}  // namespace
}  // namespace capi
}  // namespace uplink_ec

extern "C" {

int ec_repair_segments_sets(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                            const uint8_t *const *pieces, const int *ntargets, const int *targets,
                            uint8_t *const *outs, size_t nstripes, int flags, int32_t *dev_status, ec_stream stream) {
    return repair_export(cc, nseg, nshares, nums, pieces, ntargets, targets, outs, nullptr, nstripes, flags, dev_status,
                         stream);
}

int ec_repair_segments_sized(const ec_ctx *cc, size_t nseg, const int *nshares, const int *nums,
                             const uint8_t *const *pieces, const int *ntargets, const int *targets,
                             uint8_t *const *outs, const size_t *nstripes, int flags, int32_t *dev_status,
                             ec_stream stream) {
    if (nseg && !nstripes) return EC_ERR_INVALID_ARG;
    return repair_export(cc, nseg, nshares, nums, pieces, ntargets, targets, outs, nstripes, 0, flags, dev_status,
                         stream);
}

}  // extern "C"
