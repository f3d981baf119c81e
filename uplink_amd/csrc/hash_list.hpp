// The list of pieces a piece-hash call works on, built from the arguments of the
// list calls (ec_blake3_pieces_list / ec_sha256_pieces_list) and of the segment
// calls (ec_hash_segments_sized / ec_sha256_segments_sized): one validation and
// one layout rule for both algorithms (ec_hash_sized.cpp, ec_sha256.cpp).
#pragma once
#include <vector>

#include "b3_list_geom.hpp"
#include "ec_internal.hpp"

namespace uplink_ec {
namespace capi {

// One piece to hash and where its 32 bytes go.
struct HashPiece {
    b3list::Piece p;
    uint8_t *hash;
};

// The list calls' pieces: piece i contiguous at pieces[i], lens[i] bytes, row i of hashes.
// npieces > 0 and the three arrays are not NULL.  Nothing is queued or written here.
inline int list_pieces(size_t npieces, const uint8_t *const *pieces, const size_t *lens, uint8_t *hashes,
                       std::vector<HashPiece> &list) {
    if (npieces > SIZE_MAX / 32) return EC_ERR_INVALID_ARG;
    list.resize(npieces);
    for (size_t i = 0; i < npieces; i++) {
        if (!pieces[i] && lens[i]) return EC_ERR_INVALID_ARG;
        list[i] = {{(uint64_t)(uintptr_t)pieces[i], (uint64_t)lens[i], 0, 0}, hashes + 32 * i};
    }
    return EC_OK;
}

// The segment calls' pieces: all n pieces of every segment with nstripes[g] > 0, rows
// [g][0..n) of hashes; with EC_FLAG_PARITY_ONLY the data pieces in place in segs[g] (runs of
// ess bytes, k*ess apart).  nseg > 0 and nstripes, pieces, hashes are not NULL.
inline int segment_pieces(const ec_ctx *c, size_t nseg, const uint8_t *const *segs, const size_t *nstripes,
                          const uint8_t *const *pieces, int flags, uint8_t *hashes, std::vector<HashPiece> &list) {
    const size_t k = c->k, n = c->n, ess = c->ess;
    const bool parity_only = (flags & EC_FLAG_PARITY_ONLY) != 0;
    if (nseg > SIZE_MAX / (32 * n)) return EC_ERR_INVALID_ARG;
    list.clear();
    list.reserve(nseg * n);
    for (size_t g = 0; g < nseg; g++) {
        if (nstripes[g] == 0) continue;
        if (nstripes[g] > (SIZE_MAX / ess) / n) return EC_ERR_UNSUPPORTED;
        const uint64_t plen = (uint64_t)nstripes[g] * ess;
        if (parity_only ? (!segs || !segs[g] || (n > k && !pieces[g])) : !pieces[g]) return EC_ERR_INVALID_ARG;
        uint8_t *h = hashes + 32 * n * g;
        for (size_t j = 0; j < n; j++) {
            if (!parity_only)
                list.push_back({{(uint64_t)(uintptr_t)pieces[g] + j * plen, plen, 0, 0}, h + 32 * j});
            else if (j < k)  // share j of every stripe of the stripe-major segment
                list.push_back({{(uint64_t)(uintptr_t)segs[g] + j * ess, plen, (uint64_t)ess, (int64_t)(k * ess)},
                                h + 32 * j});
            else
                list.push_back({{(uint64_t)(uintptr_t)pieces[g] + (j - k) * plen, plen, 0, 0}, h + 32 * j});
        }
    }
    return EC_OK;
}

}  // namespace capi
}  // namespace uplink_ec
