// Stand-alone program over uplink_amd/csrc/enc_sized_geom.hpp (no HIP): the
// compile-time encoder's blocks per segment and each segment's first block, the
// tiles of an odd and an even block count, PadReader's padding and its check at
// the stripe boundaries, and the pass split at 1024 segments.  Built with the
// host compiler under -fsanitize=address,undefined by
// tests/test_encode_sized_host.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "enc_sized_geom.hpp"

using namespace uplink_ec::sized;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    // RS(29,80) ess 256: 16 chunks per stripe, a block is 4 stripes
    const int ess = 256;
    const uint64_t stripes[] = {1, 3, 4, 5, 8, 9, 41, 130};
    const int64_t want_blocks[] = {1, 1, 1, 2, 2, 3, 11, 33};
    std::vector<int64_t> blocks;
    for (size_t i = 0; i < 8; i++) {
        const int64_t c = chunks_of(stripes[i], ess);
        CHECK(c == (int64_t)stripes[i] * 16);
        CHECK(blocks_of(c) == want_blocks[i]);
        blocks.push_back(blocks_of(c));
    }
    CHECK(blocks_of(0) == 0 && blocks_of(1) == 1 && blocks_of(64) == 1 && blocks_of(65) == 2);
    CHECK(blocks_of(0xFFFFFFFFll) == (1ll << 26));
    // ess 4096: a block is a quarter stripe; ess 16: 64 stripes
    CHECK(blocks_of(chunks_of(1, 4096)) == 4 && blocks_of(chunks_of(3, 4096)) == 12);
    CHECK(blocks_of(chunks_of(63, 16)) == 1 && blocks_of(chunks_of(64, 16)) == 1 && blocks_of(chunks_of(65, 16)) == 2);
    // the 32-bit chunk limit
    CHECK(chunks_of((uint64_t)1 << 62, ess) == -1);
    CHECK(chunks_of(0xFFFFFFFFull / 16 + 1, ess) == -1 && chunks_of(0xFFFFFFFFull / 16, ess) > 0);
    // each segment's first block, and the total
    std::vector<int64_t> b0(blocks.size());
    const int64_t total = first_blocks(blocks.data(), blocks.size(), b0.data());
    CHECK(total == 54);
    const int64_t want_b0[] = {0, 1, 2, 3, 5, 7, 10, 21};
    for (size_t i = 0; i < 8; i++) CHECK(b0[i] == want_b0[i]);
    CHECK(first_blocks(blocks.data(), 0, b0.data()) == 0);
    // tiles: an even and an odd count; one block alone
    CHECK(pair_count(54) == 27 && pair_count(53) == 27 && pair_count(1) == 1 && pair_count(0) == 0 && pair_count(2) == 1);
    // the second block of tile t is t + pair_count: for 53 blocks the last tile (26) has none
    CHECK(26 + pair_count(53) == 53 && 26 + pair_count(54) == 53);
    // PadReader: stripe 7424
    const uint64_t st = 29 * 256;
    CHECK(pad_amount(0, st) == st);
    CHECK(pad_amount(1, st) == st - 1);
    CHECK(pad_amount(st - 5, st) == 5);
    CHECK(pad_amount(st - 4, st) == 4);
    CHECK(pad_amount(st - 3, st) == st + 3);
    CHECK(pad_amount(st, st) == st);
    CHECK(pad_amount(3 * st + 17, st) == st - 17);
    CHECK(pad_amount(7419, st) == 5 && pad_amount(7420, st) == 4 && pad_amount(100000, st) == 14 * st - 100000);
    CHECK(pad_amount(5, 0) == 0 && pad_amount(UINT64_MAX - 2, st) == 0 && pad_amount(UINT64_MAX - st - 3, st) == 0);
    CHECK(pad_matches(0, 1, st) && !pad_matches(0, 0, st) && !pad_matches(0, 2, st));
    CHECK(pad_matches(1, 1, st) && pad_matches(st - 5, 1, st) && pad_matches(st - 4, 1, st));
    CHECK(!pad_matches(st - 3, 1, st) && pad_matches(st - 3, 2, st) && !pad_matches(st - 3, 3, st));
    CHECK(pad_matches(st, 2, st) && !pad_matches(st, 1, st));
    CHECK(pad_matches(3 * st + 17, 4, st) && !pad_matches(3 * st + 17, 5, st) && !pad_matches(3 * st + 17, 3, st));
    CHECK(!pad_matches(1, UINT64_MAX, st) && !pad_matches(UINT64_MAX, 1, st) && !pad_matches(1, 1, 0));
    // passes: at most kPassSegs segments and kPassTiles map entries (blocks here)
    std::vector<int64_t> ones(1100, 1);
    std::vector<Pass> p = split_passes(ones.data(), ones.size(), kPassSegs, kPassTiles);
    CHECK(p.size() == 2 && p[0].i0 == 0 && p[0].i1 == 1024 && p[1].i0 == 1024 && p[1].i1 == 1100);
    ones.resize(1024);
    p = split_passes(ones.data(), ones.size(), kPassSegs, kPassTiles);
    CHECK(p.size() == 1 && p[0].i1 == 1024);
    std::vector<int64_t> big = {kPassTiles - 1, 1, 1, kPassTiles + 5, 2};
    p = split_passes(big.data(), big.size(), kPassSegs, kPassTiles);
    CHECK(p.size() == 4 && p[0].i1 == 2 && p[1].i1 == 3 && p[2].i1 == 4 && p[3].i1 == 5);
    CHECK(split_passes(big.data(), 0, kPassSegs, kPassTiles).empty());
    puts("ok");
    return 0;
}
