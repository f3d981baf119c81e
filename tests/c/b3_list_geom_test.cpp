// Stand-alone program over uplink_amd/csrc/b3_list_geom.hpp (no HIP): chunks,
// groups and node slots of a piece at the chunk, group and 64-MiB edges, the
// layout of a pass (first workgroup and first node slot per piece, the
// workgroup -> piece map covering every workgroup exactly once, the parents
// list) for a list in both orders, the fast / byte / oversize classification by
// alignment and run, and the pass split.  Built with the host compiler under
// -fsanitize=address,undefined by tests/test_hash_sized_host.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "b3_list_geom.hpp"

using namespace uplink_ec::b3list;
using uplink_ec::sized::Pass;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// every workgroup of both launches is mapped exactly once, to the piece whose range holds it
static int check_layout(const std::vector<Piece> &ps) {
    std::vector<Class> cls;
    for (const Piece &p : ps) cls.push_back(classify(p));
    const Layout L = layout(ps.data(), cls.data(), ps.size());
    uint64_t want[2] = {0, 0}, nodes = 0, parents = 0;
    for (size_t i = 0; i < ps.size(); i++) {
        if (cls[i] == kOversize) {
            CHECK(L.groups[i] == 0 && L.node0[i] == kNone);
            continue;
        }
        CHECK(L.groups[i] == groups_of(ps[i].len));
        CHECK(L.wg0[i] == want[cls[i]]);  // in list order within its class
        want[cls[i]] += L.groups[i];
        if (L.groups[i] > 1) {
            CHECK(L.node0[i] == nodes);
            nodes += L.groups[i];
            CHECK(L.parents[parents++] == i);
        } else {
            CHECK(L.node0[i] == kNone);
        }
    }
    CHECK(L.wgs[0] == want[0] && L.wgs[1] == want[1] && L.nodes == nodes && L.parents.size() == parents);
    CHECK(L.map.size() == want[0] + want[1]);
    CHECK(L.first(kFast) == 0 && L.first(kByte) == L.wgs[0]);
    std::vector<uint32_t> seen(ps.size(), 0);
    for (int c = 0; c < 2; c++)
        for (uint32_t w = 0; w < L.wgs[c]; w++) {
            const uint32_t i = L.map[L.first((Class)c) + w];
            CHECK(i < ps.size() && cls[i] == c);
            CHECK(w >= L.wg0[i] && w < L.wg0[i] + L.groups[i]);  // the piece's group w - wg0
            seen[i]++;
        }
    for (size_t i = 0; i < ps.size(); i++) CHECK(seen[i] == L.groups[i]);
    return 0;
}

int main() {
    const uint64_t KiB = 1024, MiB = 1024 * 1024;
    // chunks, groups, node slots
    struct {
        uint64_t len, chunks, groups, nodes;
    } t[] = {{0, 1, 1, 0},
             {1, 1, 1, 0},
             {1024, 1, 1, 0},
             {1025, 2, 1, 0},
             {256 * KiB, 256, 1, 0},
             {256 * KiB + 1, 257, 2, 2},
             {64 * MiB, 65536, 256, 256},
             {64 * MiB + 1, 65537, 257, 257}};
    for (auto &e : t) {
        CHECK(chunks_of(e.len) == e.chunks);
        CHECK(groups_of(e.len) == e.groups);
        CHECK(node_slots(e.len) == e.nodes);
        CHECK((classify({4096, e.len, 0, 0}) == kOversize) == (e.len == 64 * MiB + 1));
    }
    CHECK(chunks_of(UINT64_MAX) == (UINT64_MAX - 1) / 1024 + 1);  // no overflow
    // fast / byte by alignment and run
    CHECK(classify({4096, 100, 0, 0}) == kFast);
    CHECK(classify({4096 + 16, 100, 0, 0}) == kFast);
    CHECK(classify({4096 + 1, 100, 0, 0}) == kByte);
    CHECK(classify({4096 + 8, 100000, 0, 0}) == kByte);
    CHECK(classify({0, 0, 0, 0}) == kFast);                       // the empty piece at NULL
    CHECK(classify({4096, 2048, 256, 29 * 256}) == kFast);        // RS(29,80) ess 256 data piece
    CHECK(classify({4096 + 256, 2048, 256, 29 * 256}) == kFast);  // share 1
    CHECK(classify({4096, 2048, 64, 4 * 64}) == kFast);           // 64-byte runs: the block path
    CHECK(classify({4096, 2048, 32, 4 * 32}) == kByte);           // runs under 64 bytes
    CHECK(classify({4096, 2048, 8, 16}) == kByte);
    CHECK(classify({4096, 2400, 24, 72}) == kByte);               // no power of two
    CHECK(classify({4096, 2304, 192, 3 * 192}) == kByte);
    CHECK(classify({4096, 2048, 64, 72}) == kByte);               // a stride that breaks 16-byte alignment
    CHECK(classify({4096, 2048, 2048, 99}) == kFast);             // one run: contiguous whatever the stride
    CHECK(classify({4096, 2048, 256, 256}) == kFast);             // k = 1: run stride == run, contiguous
    CHECK(classify({4096 + 1, 64 * MiB + 1, 0, 0}) == kOversize);
    // runs as the kernels take them
    Run r = run_of({4096, 2048, 256, 29 * 256});
    CHECK(r.run == 256 && r.run_stride == 29 * 256 && r.run_shift == 8);
    r = run_of({4096, 2048, 0, 0});
    CHECK(r.run == (1ull << 62) && r.run_stride == 0 && r.run_shift == 62);
    r = run_of({4096, 2048, 4096, 8192});
    CHECK(r.run == (1ull << 62) && r.run_stride == 0);
    r = run_of({4096, 2400, 24, 72});
    CHECK(r.run == 24 && r.run_stride == 72 && r.run_shift == -1);
    r = run_of({4096, 2048, 64, 256});
    CHECK(r.run_shift == 6);
    // a pass's layout, in both orders: aligned and odd addresses, every group edge, an oversize piece inside
    const uint64_t lens[] = {0, 1, 1024, 1025, 256 * KiB, 256 * KiB + 1, 64 * MiB, 64 * MiB + 1, 257 * KiB, 2319360};
    std::vector<Piece> ps;
    uint64_t at = 1 << 20;
    for (size_t i = 0; i < sizeof lens / sizeof *lens; i++) {
        ps.push_back({at + (i % 3 == 2 ? 1 : 0), lens[i], 0, 0});
        at += (lens[i] + 64 + 15) / 16 * 16;
    }
    ps.push_back({at, 1040 * KiB, 256, 29 * 256});  // a strided data piece of five groups
    if (check_layout(ps)) return 1;
    std::vector<Piece> rev(ps.rbegin(), ps.rend());
    if (check_layout(rev)) return 1;
    if (check_layout({})) return 1;
    {
        std::vector<Class> cls;
        for (const Piece &p : ps) cls.push_back(classify(p));
        const Layout L = layout(ps.data(), cls.data(), ps.size());
        // positions 2, 5, 8 (1024, 256K + 1, 257K) start at odd addresses: bytewise; 2319360 bytes are 9 groups
        CHECK(L.wgs[0] == 1 + 1 + 1 + 1 + 256 + 9 + 5 && L.wgs[1] == 1 + 2 + 2);
        CHECK(L.nodes == 2 + 256 + 2 + 9 + 5 && L.parents.size() == 5);
    }
    // passes: bounded pieces and groups; an oversize piece counts no group
    std::vector<Piece> many(kPassPieces + 5, Piece{4096, 100, 0, 0});
    std::vector<Class> mc(many.size(), kFast);
    std::vector<Pass> p = split(many.data(), mc.data(), many.size());
    CHECK(p.size() == 2 && p[0].i0 == 0 && p[0].i1 == kPassPieces && p[1].i1 == many.size());
    std::vector<Piece> big = {{4096, 64 * MiB, 0, 0}, {4096, 64 * MiB, 0, 0}, {4096, 64 * MiB + 1, 0, 0},
                              {4096, 64 * MiB, 0, 0}, {4096, 1, 0, 0}};
    std::vector<Class> bc;
    for (const Piece &q : big) bc.push_back(classify(q));
    p = split(big.data(), bc.data(), big.size(), kPassPieces, 512);
    CHECK(p.size() == 2 && p[0].i1 == 3 && p[1].i0 == 3 && p[1].i1 == 5);  // 256 + 256 + 0 | 256 + 1
    p = split(big.data(), bc.data(), big.size(), 2, 1 << 20);
    CHECK(p.size() == 3 && p[0].i1 == 2 && p[1].i1 == 4 && p[2].i1 == 5);
    CHECK(split(big.data(), bc.data(), 0).empty());
    // one pass's counts fit 32 bits
    CHECK(kPassGroups + (int64_t)kMaxGroups < (int64_t)1 << 31);
    puts("ok");
    return 0;
}
