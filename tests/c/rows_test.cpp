// Stand-alone check of uplink_amd/csrc/rs_rows.hpp (no HIP): the partition of a
// segment's rows over passes and wave groups, pack_rows against a per-entry
// restatement of the leaf table's order, and solve_rows against codewords of the
// oracle's encoder (oracle/infectious_oracle.c, linked in).  Compiled with
// -fsanitize=address,undefined and run by tests/test_rows_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rs_rows.hpp"

extern "C" {
int or_new_fec(int k, int n, uint8_t *enc_matrix, uint8_t *vand_matrix);
int or_encode(int k, int n, const uint8_t *enc, const uint8_t *in, size_t in_len, uint8_t *out);
}

using namespace uplink_ec;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            failures++;                                              \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)

// the groups' row ranges partition 0..rows in order, at most kRows rows per group and pass
static void check_partition(int rows, int nw) {
    const int npass = npass_of(rows, nw);
    CHECK(npass >= 1 && (rows == 0 || (npass - 1) * nw * kRows < rows));
    int next = 0;
    for (int pass = 0; pass < npass; pass++)
        for (int g = 0; g < nw; g++) {
            int rb = -1, cn = -1;
            rows_of(pass, npass, rows, nw, g, rb, cn);
            CHECK(cn >= 0 && cn <= kRows);
            CHECK(cn == 0 || rb == next);
            next += cn;
        }
    CHECK(next == rows);
}

// entry [pass][j][g][o] of the table: with cn rows of group g in that pass, entry o holds the
// coefficient of input j in row rb + o - (kRows - cn), or zero when o < kRows - cn
static void check_pack(int rows, int nw, int nin, std::mt19937 &rng) {
    std::vector<uint8_t> M((size_t)(rows > 0 ? rows : 1) * nin);
    for (auto &x : M) x = (uint8_t)(1 + rng() % 255);  // never zero: a missing coefficient shows
    const size_t n = staged_entries(nin, rows, nw);
    CHECK(n % 16 == 0 && n >= leaf_entries(nin, rows, nw) && n < leaf_entries(nin, rows, nw) + 16);
    std::vector<uint8_t> out(n, 0xAA);
    pack_rows(M.data(), rows, nin, nw, out.data());
    const int npass = npass_of(rows, nw);
    CHECK(leaf_entries(nin, rows, nw) == (size_t)npass * nin * nw * kRows);
    size_t e = 0;
    for (int pass = 0; pass < npass; pass++)
        for (int j = 0; j < nin; j++)
            for (int g = 0; g < nw; g++) {
                int rb, cn;
                rows_of(pass, npass, rows, nw, g, rb, cn);
                for (int o = 0; o < kRows; o++, e++) {
                    const int r = rb + o - (kRows - cn);
                    const uint8_t want = o >= kRows - cn ? M[(size_t)r * nin + j] : 0;
                    CHECK(out[e] == want);
                }
            }
    for (; e < n; e++) CHECK(out[e] == 0);
}

static uint8_t dot(const uint8_t *row, const std::vector<const uint8_t *> &in, int nin, size_t col) {
    uint8_t acc = 0;
    for (int j = 0; j < nin; j++) acc ^= gf_mul(row[j], in[j][col]);
    return acc;
}

// each stored row applied to the basis shares of a random codeword gives the target share, and
// each syndrome row over all inputs gives zero
static void check_solve(int k, int n, std::mt19937 &rng) {
    const size_t ess = 32;
    std::vector<uint8_t> enc((size_t)n * k), data(k * ess), shares(n * ess);
    CHECK(or_new_fec(k, n, enc.data(), nullptr) == 0);
    for (auto &x : data) x = (uint8_t)rng();
    CHECK(or_encode(k, n, enc.data(), data.data(), data.size(), shares.data()) == 0);
    for (int trial = 0; trial < 8; trial++) {
        std::vector<int> perm(n);
        for (int i = 0; i < n; i++) perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        // inputs: k basis shares, then up to 4 others; targets: every share that is no input, and
        // one that is a basis share (a unit row)
        const int extra = trial % 2 ? std::min(4, n - k) : 0, nin = k + extra;
        std::vector<int> num(perm.begin(), perm.begin() + nin), targets(perm.begin() + nin, perm.end());
        targets.push_back(num[trial % k]);
        const int nt = (int)targets.size(), rows = nt + extra;
        std::vector<uint8_t> M((size_t)rows * nin, 0x55);
        solve_rows(num.data(), k, nin, targets.data(), nt, M.data());
        std::vector<const uint8_t *> in;
        for (int j = 0; j < nin; j++) in.push_back(&shares[(size_t)num[j] * ess]);
        for (int r = 0; r < rows; r++)
            for (size_t col = 0; col < ess; col++) {
                const uint8_t got = dot(&M[(size_t)r * nin], in, nin, col);
                CHECK(got == (r < nt ? shares[(size_t)targets[r] * ess + col] : 0));
            }
        for (int r = 0; r < nt; r++)  // stored rows read the basis only
            for (int j = k; j < nin; j++) CHECK(M[(size_t)r * nin + j] == 0);
    }
}

int main() {
    std::mt19937 rng(20261020);
    for (int nw : {2, 3, 4, 8})
        for (int rows = 0; rows <= 64; rows++) {
            check_partition(rows, nw);
            for (int nin : {1, 2, 29, 30, 58}) check_pack(rows, nw, nin, rng);
        }
    check_solve(4, 10, rng);
    check_solve(29, 80, rng);
    if (failures) return 1;
    puts("ok");
    return 0;
}
