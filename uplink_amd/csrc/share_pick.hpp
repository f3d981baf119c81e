// Which shares of a segment the share-set calls read, and in what order:
// infectious Rebuild's choice of k, then -- where the caller checks the others
// against them -- the rest by number.  Plain C++, no HIP, no context:
// tests/test_share_pick_host.py compiles it on its own.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/uplink_ec.h"

namespace uplink_ec {

// infectious Rebuild's share choice over the list nums[0..nshares), nshares >= k:
// sort by number (stable), then for i in 0..k-1 take the front share if its
// number == i else take from the back.  pos[i] / num[i]: the list position and
// the number of basis slot i.  On return order[b..e] holds the positions not
// taken, by number, equal numbers in list order.
inline int front_back(int k, int n, int nshares, const int *nums, std::vector<int> &order, int *pos, int *num, int &b,
                      int &e) {
    order.resize(nshares);
    for (int i = 0; i < nshares; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return nums[x] < nums[y]; });
    b = 0, e = nshares - 1;
    for (int i = 0; i < k; i++) {
        const int pick = nums[order[b]] == i ? order[b++] : order[e--];
        if (nums[pick] >= n || nums[pick] < 0) return EC_ERR_INVALID_SHARE;
        pos[i] = pick;
        num[i] = nums[pick];
    }
    return EC_OK;
}

// The choice alone: the k list positions and their numbers.
inline int choose_shares(int k, int n, int nshares, const int *nums, std::vector<int> &order_out,
                         std::vector<int> &ids_out) {
    if (nshares < k) return EC_ERR_NOT_ENOUGH_SHARES;
    order_out.resize(k);
    ids_out.resize(k);
    std::vector<int> order;
    int b, e;
    return front_back(k, n, nshares, nums, order, order_out.data(), ids_out.data(), b, e);
}

// A segment's inputs in the kernels' order: the k chosen shares, then -- with
// `rest` -- the others by number (stable).  pos / num: list positions and
// numbers, nin of them (k, or nshares with `rest`: the caller's storage holds
// that many); missing (k entries, or null): the nmissing basis slots that hold a
// parity share, the data positions to compute.  Errors in Rebuild's order: too
// few shares; a number out of range, among the chosen k or -- all_valid, as
// Decode checks them -- among all; a number chosen twice (singular).
inline int pick_inputs(int k, int n, int nshares, const int *nums, bool all_valid, bool rest, int *pos, int *num,
                       int *missing, int &nin, int &nmissing) {
    if (nshares < k) return EC_ERR_NOT_ENOUGH_SHARES;
    for (int i = 0; i < nshares && all_valid; i++)
        if (nums[i] < 0 || nums[i] >= n) return EC_ERR_INVALID_SHARE;
    std::vector<int> order;
    int b, e;
    if (int rc = front_back(k, n, nshares, nums, order, pos, num, b, e)) return rc;
    bool seen[256] = {};
    nmissing = 0;
    for (int i = 0; i < k; i++) {
        if (seen[num[i]]) return EC_ERR_SINGULAR;
        seen[num[i]] = true;
        if (missing && num[i] >= k) missing[nmissing++] = i;
    }
    nin = k;
    for (int q = b; q <= e && rest; q++) {
        pos[nin] = order[q];
        num[nin++] = nums[order[q]];
    }
    return EC_OK;
}

}  // namespace uplink_ec
