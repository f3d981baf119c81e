// Stand-alone program over uplink_amd/csrc/gcm_sized_geom.hpp (no HIP): the
// workgroups of a segment at the block-count edges and in the capped regime, the
// layout of a pass (first workgroup per segment, the workgroup -> segment map
// covering every workgroup exactly once) for a list in both orders, the kernel's
// stride loop visiting every block of a segment exactly once, the pass split,
// PadReader's rule at every residue edge and the sizes of an upload through the
// cipher.  Built with the host compiler under -fsanitize=address,undefined by
// tests/test_gcm_sized_host.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gcm_sized_geom.hpp"

using namespace uplink_ec::gcmsized;
using uplink_ec::sized::Pass;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// every workgroup is mapped exactly once, to the segment whose range holds it; every (workgroup,
// wave, iteration) of the stride loop visits a block of its segment, and every block exactly once
static int check_layout(const std::vector<uint64_t> &nb, uint32_t T) {
    const Layout L = layout(nb.data(), nb.size(), T);
    uint64_t total = 0, grid = 0;
    for (uint64_t x : nb) total += x;
    CHECK(L.total_blocks == total);
    for (size_t i = 0; i < nb.size(); i++) {
        CHECK(L.wg0[i] == grid);  // in list order
        CHECK(L.wgs[i] == wgs_of(nb[i], total, T));
        CHECK((L.wgs[i] == 0) == (nb[i] == 0));  // nobody at 0 who has blocks
        CHECK(L.wgs[i] <= (nb[i] + 3) / 4);      // no workgroup without a block
        grid += L.wgs[i];
    }
    CHECK(L.map.size() == grid);
    CHECK(grid <= (uint64_t)T + nb.size());
    std::vector<uint32_t> seen(nb.size(), 0);
    for (uint32_t w = 0; w < L.map.size(); w++) {
        const uint32_t i = L.map[w];
        CHECK(i < nb.size());
        CHECK(w >= L.wg0[i] && w < L.wg0[i] + L.wgs[i]);
        seen[i]++;
    }
    for (size_t i = 0; i < nb.size(); i++) CHECK(seen[i] == L.wgs[i]);
    for (size_t i = 0; i < nb.size(); i++) {
        std::vector<uint8_t> hit(nb[i], 0);
        bool ok = true;
        for (uint32_t wg = 0; wg < L.wgs[i]; wg++)
            for (uint32_t wave = 0; wave < kWaves; wave++)
                for_blocks(wg, wave, L.wgs[i], (uint32_t)nb[i], [&](uint32_t b) {
                    if (b >= nb[i] || hit[b]) ok = false;
                    else hit[b] = 1;
                });
        CHECK(ok);
        for (uint64_t b = 0; b < nb[i]; b++) CHECK(hit[b] == 1);
    }
    return 0;
}

int main() {
    // a pass smaller than the grid: every wave at most one block
    const uint32_t T = 256 * 32;
    struct {
        uint64_t nblocks;
        uint32_t wgs;
    } t[] = {{0, 0}, {1, 1}, {3, 1}, {4, 1}, {5, 2}, {8, 2}, {9, 3}};
    uint64_t total = 0;
    for (auto &e : t) total += e.nblocks;
    for (auto &e : t) CHECK(wgs_of(e.nblocks, total, T) == e.wgs);
    CHECK(wgs_of(1, 1, T) == 1 && wgs_of(0, 0, T) == 0);
    CHECK(wgs_of(0x7FFFFFFFu, 0x7FFFFFFFull * 4096, 256 * 64) == 4);      // no overflow at the limits
    CHECK(wgs_of(0x7FFFFFFFu, 0x7FFFFFFFu, 256 * 64) == 256 * 64);          // one huge segment: the whole grid
    // the capped regime: T = 8 with segments of 1, 5 and 1000 blocks
    {
        const uint64_t nb[] = {1, 5, 1000};
        const Layout L = layout(nb, 3, 8);
        CHECK(L.wgs[0] == 1 && L.wgs[1] == 1 && L.wgs[2] == 8);  // ceil(8/1006), ceil(40/1006), ceil(8000/1006)
        CHECK(L.map.size() <= 8 + 3);
        CHECK(L.wg0[0] == 0 && L.wg0[1] == 1 && L.wg0[2] == 2);
    }
    const std::vector<uint64_t> edge = {1, 3, 4, 5, 0, 8, 9, 41, 130};
    const std::vector<uint64_t> redge(edge.rbegin(), edge.rend());
    for (uint32_t grid : {8u, 256u, T}) {
        if (check_layout(edge, grid) || check_layout(redge, grid)) return 1;
        if (check_layout({1, 5, 1000}, grid) || check_layout({1000, 5, 1}, grid)) return 1;
        if (check_layout({1, 40000, 5, 700}, grid)) return 1;
    }
    if (check_layout({}, T) || check_layout({0, 0}, T)) return 1;
    // the pass split
    std::vector<Pass> p = split(4096);
    CHECK(p.size() == 1 && p[0].i0 == 0 && p[0].i1 == 4096);
    p = split(4097);
    CHECK(p.size() == 2 && p[0].i1 == 4096 && p[1].i0 == 4096 && p[1].i1 == 4097);
    p = split(5, 2);
    CHECK(p.size() == 3 && p[0].i1 == 2 && p[1].i1 == 4 && p[2].i1 == 5);
    CHECK(split(0).empty());
    CHECK(kPassSegs == 4096);
    // PadReader's rule at every residue edge of a 7408-byte block
    const uint64_t ib = 7408;
    struct {
        uint64_t len, pad, nblocks;
    } d[] = {{0, 7408, 1},         {1, 7407, 1},         {7403, 5, 1},          {7404, 4, 1},
             {7405, 7411, 2},      {7408, 7408, 2},      {2 * 7408 - 4, 4, 2},  {2 * 7408 - 3, 7411, 3},
             {100000, 3712, 14}};
    for (auto &e : d) {
        CHECK(pad_amount(e.len, ib) == e.pad);
        CHECK((e.len + e.pad) % ib == 0 && e.pad >= 4 && e.pad < ib + 4);
        CHECK(pad_matches(e.len, e.nblocks, ib));
        CHECK(!pad_matches(e.len, e.nblocks + 1, ib) && !pad_matches(e.len, e.nblocks - 1, ib));
        const CipherSizes s = cipher_sizes(e.len, ib);
        CHECK(s.nblocks == e.nblocks && s.plain_cap == e.nblocks * ib && s.enc_len == e.nblocks * (ib + 16));
    }
    CHECK(pad_amount(12, 16) == 4 && pad_amount(13, 16) == 19 && pad_amount(0, 16) == 16);
    CHECK(!pad_matches(UINT64_MAX - 3, 1, ib) && !pad_matches(0, UINT64_MAX, ib) && !pad_matches(0, 0, ib));
    CHECK(cipher_sizes(UINT64_MAX - 10, ib).nblocks == 0);
    CHECK(cipher_sizes(67108864, ib).nblocks == 9059);  // a 64 MiB segment
    puts("ok");
    return 0;
}
