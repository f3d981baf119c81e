// Stand-alone check of uplink_amd/csrc/share_pick.hpp (no HIP) against the
// oracle's Rebuild (oracle/infectious_oracle.c, linked in): the k shares picked
// are the k the oracle reads -- garbage in every other share leaves its output
// as it was, a flipped byte in any picked one changes it -- and the rest are the
// unpicked shares by number.  Compiled with -fsanitize=address,undefined and run
// by tests/test_share_pick_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "share_pick.hpp"

extern "C" {
int or_new_fec(int k, int n, uint8_t *enc_matrix, uint8_t *vand_matrix);
int or_encode(int k, int n, const uint8_t *enc, const uint8_t *in, size_t in_len, uint8_t *out);
int or_rebuild(int k, int n, const uint8_t *enc, int ns, int *numbers, const uint8_t **data, size_t len, uint8_t *out);
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

constexpr size_t kLen = 32;  // bytes per share

struct Code {
    int k, n;
    std::vector<uint8_t> enc;
    Code(int k_, int n_) : k(k_), n(n_), enc((size_t)n_ * k_) { CHECK(or_new_fec(k, n, enc.data(), nullptr) == 0); }
};

// the oracle's Rebuild of the list (it sorts its arguments: copies)
static int oracle_rebuild(const Code &c, const std::vector<int> &nums, const std::vector<std::vector<uint8_t>> &bytes,
                          std::vector<uint8_t> &out) {
    std::vector<int> num(nums);
    std::vector<const uint8_t *> ptr;
    for (auto &b : bytes) ptr.push_back(b.data());
    out.assign((size_t)c.k * kLen, 0);
    return or_rebuild(c.k, c.n, c.enc.data(), (int)num.size(), num.data(), ptr.data(), kLen, out.data());
}

struct Pick {
    int rc, nin = 0, nmissing = 0;
    std::vector<int> pos, num, missing;
};

static Pick pick(const Code &c, const std::vector<int> &nums, bool all_valid, bool rest) {
    const int ns = (int)nums.size();
    Pick p;
    p.pos.assign(std::max(ns, c.k), -1);
    p.num.assign(std::max(ns, c.k), -1);
    p.missing.assign(c.k, -1);
    p.rc = pick_inputs(c.k, c.n, ns, nums.data(), all_valid, rest, p.pos.data(), p.num.data(), p.missing.data(), p.nin,
                       p.nmissing);
    return p;
}

// A list the pick accepts (numbers in range wherever the oracle looks): the
// picked k are the oracle's, `missing` and the rest are as documented.  Returns
// the pick.
static Pick check_list(const Code &c, const std::vector<int> &nums, std::mt19937 &rng) {
    const int k = c.k, ns = (int)nums.size();
    std::vector<uint8_t> data((size_t)k * kLen), shares((size_t)c.n * kLen);
    for (auto &x : data) x = (uint8_t)rng();
    CHECK(or_encode(k, c.n, c.enc.data(), data.data(), data.size(), shares.data()) == 0);
    const Pick p = pick(c, nums, false, true);
    CHECK(p.rc == EC_OK && p.nin == ns);
    if (p.rc != EC_OK) return p;
    // without the rest: the same k, nothing more
    const Pick p0 = pick(c, nums, false, false);
    CHECK(p0.rc == EC_OK && p0.nin == k && p0.nmissing == p.nmissing);
    for (int i = 0; i < k; i++) CHECK(p0.pos[i] == p.pos[i] && p0.num[i] == p.num[i]);
    std::vector<int> order, ids;
    CHECK(choose_shares(k, c.n, ns, nums.data(), order, ids) == EC_OK && (int)order.size() == k && (int)ids.size() == k);
    for (int i = 0; i < k; i++) CHECK(order[i] == p.pos[i] && ids[i] == p.num[i]);
    // every share that is not picked holds random bytes: the oracle still returns the data
    std::vector<char> picked(ns, 0);
    for (int i = 0; i < k; i++) {
        CHECK(p.pos[i] >= 0 && p.pos[i] < ns && !picked[p.pos[i]] && p.num[i] == nums[p.pos[i]]);
        picked[p.pos[i]] = 1;
    }
    std::vector<std::vector<uint8_t>> bytes(ns, std::vector<uint8_t>(kLen));
    for (int i = 0; i < ns; i++)
        for (size_t b = 0; b < kLen; b++)
            bytes[i][b] = picked[i] ? shares[(size_t)nums[i] * kLen + b] : (uint8_t)rng();
    std::vector<uint8_t> out, out2;
    CHECK(oracle_rebuild(c, nums, bytes, out) == 0);
    CHECK(out == data);
    // a byte flipped in any picked share changes its output: the oracle reads exactly our k
    for (int i = 0; i < k; i++) {
        uint8_t &byte = bytes[p.pos[i]][rng() % kLen];
        byte ^= 0x5A;
        CHECK(oracle_rebuild(c, nums, bytes, out2) == 0);
        CHECK(out2 != data);
        byte ^= 0x5A;
    }
    // missing: the basis slots that hold a parity share, in order
    int m = 0;
    for (int i = 0; i < k; i++)
        if (p.num[i] >= k) CHECK(m < p.nmissing && p.missing[m++] == i);
    CHECK(m == p.nmissing);
    // the rest: every unpicked position once, numbers non-decreasing, equal numbers in list order
    for (int j = k; j < ns; j++) {
        CHECK(p.pos[j] >= 0 && p.pos[j] < ns && !picked[p.pos[j]] && p.num[j] == nums[p.pos[j]]);
        picked[p.pos[j]] = 1;
        if (j > k) CHECK(p.num[j - 1] < p.num[j] || (p.num[j - 1] == p.num[j] && p.pos[j - 1] < p.pos[j]));
    }
    return p;
}

// every subset of 0..n-1 of size k..n: sorted, reversed and three shuffles
static void all_subsets(const Code &c, std::mt19937 &rng) {
    for (unsigned mask = 0; mask < (1u << c.n); mask++) {
        std::vector<int> nums;
        for (int i = 0; i < c.n; i++)
            if (mask >> i & 1) nums.push_back(i);
        if ((int)nums.size() < c.k) continue;
        check_list(c, nums, rng);
        std::reverse(nums.begin(), nums.end());
        check_list(c, nums, rng);
        for (int t = 0; t < 3; t++) {
            std::shuffle(nums.begin(), nums.end(), rng);
            check_list(c, nums, rng);
        }
    }
}

static void random_lists(const Code &c, int count, std::mt19937 &rng) {
    std::vector<int> perm(c.n);
    for (int i = 0; i < c.n; i++) perm[i] = i;
    for (int t = 0; t < count; t++) {
        std::shuffle(perm.begin(), perm.end(), rng);
        const int ns = c.k + (int)(rng() % (unsigned)(c.n - c.k + 1));
        check_list(c, std::vector<int>(perm.begin(), perm.begin() + ns), rng);
    }
}

// a list the pick refuses with `want`, whatever is asked of it; the oracle's code is `want_oracle`
static void check_refused(const Code &c, const std::vector<int> &nums, int want_oracle, int want) {
    std::vector<std::vector<uint8_t>> bytes(nums.size(), std::vector<uint8_t>(kLen, 0x11));
    std::vector<uint8_t> out;
    CHECK(oracle_rebuild(c, nums, bytes, out) == want_oracle);
    for (int all_valid = 0; all_valid < 2; all_valid++)
        for (int rest = 0; rest < 2; rest++) CHECK(pick(c, nums, all_valid, rest).rc == want);
    if (want != EC_ERR_SINGULAR) {  // (the choice alone does not look for a repeated number)
        std::vector<int> order, ids;
        CHECK(choose_shares(c.k, c.n, (int)nums.size(), nums.data(), order, ids) == want);
    }
}

static void error_lists(std::mt19937 &rng) {
    const Code c(4, 10);
    // out of range among the picked
    check_refused(c, {0, 1, 2, 10}, -11, EC_ERR_INVALID_SHARE);
    check_refused(c, {10, 7, 0, 5}, -11, EC_ERR_INVALID_SHARE);
    check_refused(c, {-1, 1, 2, 3}, -11, EC_ERR_INVALID_SHARE);
    check_refused(c, {3, 8, -1, 6}, -11, EC_ERR_INVALID_SHARE);
    // out of range and not picked: Rebuild does not look at it; whoever checks all shares refuses
    for (const std::vector<int> &nums : {std::vector<int>{0, 1, 2, 3, 10}, std::vector<int>{3, -1, 0, 2, 1}}) {
        std::vector<std::vector<uint8_t>> bytes(nums.size(), std::vector<uint8_t>(kLen, 0x11));
        std::vector<uint8_t> out;
        CHECK(oracle_rebuild(c, nums, bytes, out) == 0);
        CHECK(pick(c, nums, false, false).rc == EC_OK);
        CHECK(pick(c, nums, true, false).rc == EC_ERR_INVALID_SHARE);
        CHECK(pick(c, nums, true, true).rc == EC_ERR_INVALID_SHARE);
    }
    // a number twice, both copies picked
    check_refused(c, {5, 6, 7, 7}, -12, EC_ERR_SINGULAR);
    check_refused(c, {0, 9, 1, 9}, -12, EC_ERR_SINGULAR);
    check_refused(c, {6, 6, 5, 5, 0}, -12, EC_ERR_SINGULAR);  // (0, then 6 6 5 from the back)
    // (a data number picked twice -- 0 1 2 from the front, the second 2 from the back into slot 3 --
    // is the one list on which the two part: the oracle, as infectious, puts a 1 on the diagonal
    // of any slot that holds a data share, inverts that and leaves data position 3 unwritten; the
    // pick refuses the list)
    check_refused(c, {2, 0, 1, 2}, 0, EC_ERR_SINGULAR);
    // a number twice, one copy left out: both accept, and the copy picked is the oracle's (check_list
    // gives the other copy random bytes).  From the front the first copy in list order is taken,
    // from the back the last.
    Pick p = check_list(c, {0, 1, 2, 3, 3}, rng);
    CHECK(p.rc == EC_OK && p.pos[3] == 3 && p.pos[4] == 4);
    p = check_list(c, {9, 9, 1, 0, 2}, rng);
    CHECK(p.rc == EC_OK && p.pos[3] == 1 && p.pos[4] == 0 && p.nmissing == 1 && p.missing[0] == 3);
    p = check_list(c, {1, 1, 0, 2, 3, 7}, rng);
    CHECK(p.rc == EC_OK && p.pos[1] == 0 && p.num[2] == 7 && p.pos[4] == 1 && p.num[4] == 1 && p.pos[5] == 3);
    // too few
    check_refused(c, {0, 1, 2}, -10, EC_ERR_NOT_ENOUGH_SHARES);
    check_refused(c, {7, 7, 10}, -10, EC_ERR_NOT_ENOUGH_SHARES);
}

int main() {
    std::mt19937 rng(20261021);
    all_subsets(Code(2, 4), rng);
    all_subsets(Code(3, 7), rng);
    random_lists(Code(4, 10), 200, rng);
    random_lists(Code(29, 80), 200, rng);
    error_lists(rng);
    if (failures) return 1;
    puts("ok");
    return 0;
}
