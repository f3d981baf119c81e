// The row layout of the share-set kernels (rs_sets_tile.hpp) and the rows the
// host solves for them: which rows a wave group computes in which pass, the
// size and order of a segment's leaf table, and a segment's matrix from its
// basis shares.  Plain C++, no HIP, read by the device header and by the host
// files alike: tests/test_rows_host.py compiles it on its own.
#pragma once
#include <cstddef>
#include <cstring>

#include "gf256_field.hpp"
#include "rs_args.hpp"

#ifdef __HIPCC__
#define UPLINK_ROWS_FN __host__ __device__ __forceinline__
#else
#define UPLINK_ROWS_FN inline
#endif

namespace uplink_ec {

constexpr int kRows = 8;  // accumulator rows per wave (jt_inputs)

// passes over the inputs that nout rows take on nw waves
UPLINK_ROWS_FN int npass_of(int nout, int nw) { return nout > 0 ? (nout + nw * kRows - 1) / (nw * kRows) : 1; }

// the rows [rbase, rbase + cnt) that group g of nw computes in pass `pass` of npass: the passes
// split the rows evenly, and so do the groups of a pass (cnt <= kRows)
UPLINK_ROWS_FN void rows_of(int pass, int npass, int nout, int nw, int g, int &rbase, int &cnt) {
    const int p0 = pass * nout / npass, prow = (pass + 1) * nout / npass - p0;
    rbase = p0 + g * prow / nw;
    cnt = p0 + (g + 1) * prow / nw - rbase;
}

// most tiles one launch of a share-set kernel on nw waves takes (one workgroup per tile, the
// grid's work-items below 2^32)
inline int64_t share_max_tiles(int nw) { return (int64_t)(0xFFFFFFFFu / (unsigned)(nw * 64)); }

// entries of one segment's leaf table on nw waves: [pass][input][group][kRows]
inline size_t leaf_entries(int nin, int rows, int nw) { return (size_t)npass_of(rows, nw) * nin * nw * kRows; }
// the same rounded up to 16: the bytes of a segment's coefficient staging and the words of its
// leaf table where a prep kernel reads 16 coefficients per load (rs_sets_tile.hpp write_leaves)
inline size_t staged_entries(int nin, int rows, int nw) { return (leaf_entries(nin, rows, nw) + 15) & ~(size_t)15; }

// The coefficients of M (rows x nin, M[r * nin + j]) in the leaf table's order,
// one byte per entry: [pass][input][group][kRows], a group's rows right-aligned,
// zero where a group has fewer than kRows rows.  `out`: staged_entries bytes.
inline void pack_rows(const uint8_t *M, int rows, int nin, int nw, uint8_t *out) {
    memset(out, 0, staged_entries(nin, rows, nw));
    const int npass = npass_of(rows, nw);
    for (int pass = 0; pass < npass; pass++)
        for (int g = 0; g < nw; g++) {
            int rb, cn;
            rows_of(pass, npass, rows, nw, g, rb, cn);
            for (int j = 0; j < nin; j++) {
                uint8_t *e = out + (((size_t)pass * nin + j) * nw + g) * kRows + (kRows - cn);
                for (int o = 0; o < cn; o++) e[o] = M[(size_t)(rb + o) * nin + j];
            }
        }
}

// Lagrange interpolation through the points of k basis shares (piece numbers
// ids[0..k)), in logarithms: the closed form of rs_sets.hip (solve_rows).
// row(y, out): out[p] = L_p(y), the coefficient of basis share p in the share
// at point y -- a unit vector when y is itself a basis point.
struct LagrangeBasis {
    int k = 0;
    uint8_t x[kMaxOps];
    int lw[kMaxOps];  // log W_p, W_p = prod over t != p of (x_p - x_t)
    LagrangeBasis(const int *ids, int k_) : k(k_) {
        for (int p = 0; p < k; p++) x[p] = gf_point(ids[p]);
        for (int p = 0; p < k; p++) {
            int l = 0;
            for (int t = 0; t < k; t++)
                if (t != p) l += kGf.log[x[p] ^ x[t]];
            lw[p] = l % 255;
        }
    }
    void row(uint8_t y, uint8_t *out) const {
        int ln = 0, hit = -1;
        for (int t = 0; t < k; t++) {
            if (y == x[t]) hit = t;
            else ln += kGf.log[y ^ x[t]];
        }
        for (int j = 0; j < k; j++)
            out[j] = hit >= 0 ? (uint8_t)(hit == j) : kGf.exp[(((ln - kGf.log[y ^ x[j]] - lw[j]) % 255) + 255) % 255];
    }
};

// A segment's matrix M (nt + nin - k rows of nin columns, M[r * nin + j]) over
// its inputs num[0..nin): the k basis shares, then the other shares.  Row r < nt
// is the share numbered targets[r] from the basis (a missing data position, a
// piece to repair); then one syndrome row per non-basis input: its prediction
// from the basis, and 1 on the input itself (the two cancel when the share agrees).
inline void solve_rows(const int *num, int k, int nin, const int *targets, int nt, uint8_t *M) {
    const LagrangeBasis L(num, k);
    const int rows = nt + nin - k;
    memset(M, 0, (size_t)rows * nin);
    for (int r = 0; r < rows; r++) {
        L.row(gf_point(r < nt ? targets[r] : num[k + r - nt]), M + (size_t)r * nin);
        if (r >= nt) M[(size_t)r * nin + k + r - nt] = 1;
    }
}

}  // namespace uplink_ec
