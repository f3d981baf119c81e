// One staged pass of a call that prepares its segments on the host (ec_sized.cpp,
// ec_repair.cpp): a block of the pool carved into the segments' records, their
// coefficients, descriptors, leaf tables and -- a pass of segments of their own
// sizes -- the classes' tile maps; per segment the fields every descriptor has
// and its rows, solved and packed; the prep launch, the caller's launches, the
// block's release.  Host only.
#pragma once
#include "ec_internal.hpp"
#include "sized_geom.hpp"

namespace uplink_ec {
namespace capi {

// What a pass's callables see of its block.
template <class Stage>
struct StagedPass {
    using Desc = decltype(Stage::d);
    Stage *stage;                // pinned: the segments' records, in the pass's order
    Desc *desc;                  // device: their descriptors (made by the prep launch)
    uint32_t *map;               // device: the classes' tile maps (a pass with a Layout)
    uint8_t *h_extra, *d_extra;  // the caller's `extra` bytes, pinned and device (4-byte aligned)
};

struct NoHook {
    template <class P>
    hipError_t operator()(const P &) const {
        return hipSuccess;
    }
};

// The pass over n segments on stream s.  seg(q): the segment at position q of
// the pass (its in, num, rows, nw; with a Layout its chunks and tiles too);
// stored: the segment's member that lists the rows it stores (the syndrome rows follow);
// L: the layout of a pass whose Stage carries a segment's own geometry, which
// sets tile0, map and ntiles from it; fill(st, sg, q, pass): the fields only
// this descriptor has, into the zeroed record; prep: the prep launcher;
// launch(pass): the tile launches; before_release(pass): after them, while the
// block is still the caller's.
template <class Stage, class SegAt, class Stored, class Fill, class Prep, class Launch, class Hook = NoHook>
int staged_pass(ec_ctx *c, StagePool &pool, size_t n, SegAt seg, Stored stored, const sized::Layout *L, size_t extra,
                Fill fill, Prep prep, Launch launch, hipStream_t s, Hook before_release = Hook{}) {
    using Desc = typename StagedPass<Stage>::Desc;
    std::vector<size_t> eoff(n + 1, 0);
    for (size_t q = 0; q < n; q++) {
        const auto &sg = seg(q);
        eoff[q + 1] = eoff[q] + staged_entries((int)sg.in.size(), sg.rows, sg.nw);
    }
    // (coefficients on 16 bytes, descriptors and leaf tables on 8, map and extra on 4)
    const size_t h_stage = up(n * sizeof(Stage), 16), d_desc = up(n * sizeof(Desc), 256), d_tgt_len = eoff[n] * 8;
    const size_t d_map_len = L ? (size_t)L->map_entries * 4 : 0;
    StageBlock *b = block_acquire(pool, h_stage + eoff[n] + extra, d_desc + d_tgt_len + d_map_len + extra);
    if (!b) return EC_ERR_DEVICE;
    uint8_t *h_coef = b->h + h_stage;
    uint64_t *d_tgt = (uint64_t *)(b->d + d_desc);
    const StagedPass<Stage> p{(Stage *)b->h, (Desc *)b->d, (uint32_t *)(b->d + d_desc + d_tgt_len), h_coef + eoff[n],
                              b->d + d_desc + d_tgt_len + d_map_len};
    std::vector<uint8_t> M;
    for (size_t q = 0; q < n; q++) {
        const auto &sg = seg(q);
        const std::vector<int> &rows = sg.*stored;
        const int nin = (int)sg.in.size(), nst = (int)rows.size();
        Stage &st = p.stage[q];
        memset(&st, 0, sizeof(st));
        for (int j = 0; j < nin; j++) st.d.in[j] = sg.in[j];
        st.d.tgt = d_tgt + eoff[q];
        st.d.nin = nin;
        st.d.nout = sg.rows;
        st.d.nstore = nst;
        st.coef = h_coef + eoff[q];
        st.entries = (int64_t)(eoff[q + 1] - eoff[q]);
        if constexpr (requires { st.map; }) {
            st.d.chunks = sg.chunks;
            st.d.piece_len = sg.chunks * 16;
            st.d.tile0 = L->tile0[q];
            st.map = p.map + L->map_off[q] + L->tile0[q];
            st.ntiles = sg.tiles;
        }
        fill(st, sg, q, p);
        // the rows (the stored ones, then the syndrome rows) in the leaf table's order
        M.resize((size_t)std::max(sg.rows, 1) * nin);
        solve_rows(sg.num.data(), c->k, nin, rows.data(), nst, M.data());
        pack_rows(M.data(), sg.rows, nin, sg.nw, h_coef + eoff[q]);
    }
    hipError_t e = prep(p.stage, p.desc, (int)n, c->jt_base, s);
    if (e != hipSuccess) {  // nothing was queued
        block_release(pool, b, false, s);
        return hip_fail(e);
    }
    e = launch(p);
    if (e == hipSuccess) e = before_release(p);
    block_release(pool, b, true, s);
    if (e != hipSuccess) return hip_fail(e);
    c->last_body = EC_BODY_JUMP_TABLE;
    return after_launch(c->d_chk, s);
}

}  // namespace capi
}  // namespace uplink_ec
