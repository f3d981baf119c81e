// Stand-alone program over uplink_amd/csrc/sha_list_geom.hpp and
// sha256_device.hpp (no HIP): blocks per piece at the padding edges, the fast /
// byte classes, the lane order of a pass (a permutation, sorted within a class,
// no wave of two classes), the pass split, the launch counts; then the very
// rounds and tail builder the kernel uses, compiled for the host: the messages
// given on the command line (tests/golden/sha256_vectors.json, handed over by
// the test as <repeat>:<unit, hex>:<digest, hex>) hashed block by block, also in
// launches with the state carried, and the tail's 64-bit length field for
// lengths no test can afford as data, from an injected state.  Built with the
// host compiler under -fsanitize=address,undefined by tests/test_sha256_host.py;
// prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sha256_device.hpp"
#include "sha_list_geom.hpp"

using namespace uplink_ec::shalist;
using uplink_ec::sized::Pass;
namespace sha = uplink_ec::sha256;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// the lanes are a permutation of the pieces plus padding; each class sorted by block count,
// descending; fast lanes first; no wave holds two classes
static int check_layout(const std::vector<Piece> &ps) {
    const Layout L = layout(ps.data(), ps.size());
    CHECK(L.lanes() % kWave == 0);
    std::vector<int> seen(ps.size(), 0);
    uint64_t maxb = 0;
    uint32_t count[2] = {0, 0};
    for (uint32_t w = 0; w < L.waves(); w++) {
        int cls = -1;
        for (uint32_t j = w * kWave; j < (w + 1) * kWave; j++) {
            const uint32_t r = L.row[j];
            if (r == kNone) continue;
            CHECK(r < ps.size());
            seen[r]++;
            const int c = class_of(ps[r]);
            CHECK(cls == -1 || cls == c);
            cls = c;
            count[c]++;
            maxb = blocks_of(ps[r].len) > maxb ? blocks_of(ps[r].len) : maxb;
        }
    }
    for (size_t i = 0; i < ps.size(); i++) CHECK(seen[i] == 1);
    CHECK(count[0] == L.count[0] && count[1] == L.count[1] && count[0] + count[1] == ps.size());
    CHECK(L.max_blocks == maxb);
    CHECK(L.lanes() == (count[0] + kWave - 1) / kWave * kWave + (count[1] + kWave - 1) / kWave * kWave);
    int last_cls = 0;
    uint64_t last_blocks = UINT64_MAX;
    uint32_t last_row = 0;
    for (uint32_t j = 0; j < L.lanes(); j++) {
        if (L.row[j] == kNone) continue;
        const Piece &p = ps[L.row[j]];
        const int c = class_of(p);
        CHECK(c >= last_cls);  // the fast class first
        if (c != last_cls) last_blocks = UINT64_MAX;
        CHECK(blocks_of(p.len) <= last_blocks);
        if (blocks_of(p.len) == last_blocks) CHECK(L.row[j] > last_row);  // ties in list order
        last_cls = c, last_blocks = blocks_of(p.len), last_row = L.row[j];
    }
    return 0;
}

// SHA-256 of p[0..len) as a lane computes it: block by block through pad_block and compress,
// in launches of launch_blocks blocks with the eight state words carried between them
static void hash_lane(const uint8_t *p, uint64_t len, uint64_t launch_blocks, uint8_t out[32]) {
    uint32_t carried[8];
    const uint64_t nb = sha::blocks_of(len);
    for (uint64_t blk0 = 0; blk0 < nb; blk0 += launch_blocks) {
        uint32_t h[8];
        for (int i = 0; i < 8; i++) h[i] = blk0 == 0 ? sha::kInit[i] : carried[i];
        const uint64_t end = nb - blk0 > launch_blocks ? blk0 + launch_blocks : nb;
        for (uint64_t b = blk0; b < end; b++) {
            uint32_t w[16] = {0};
            for (uint64_t i = 0; i < 64; i++)
                if (64 * b + i < len) w[i / 4] |= (uint32_t)p[64 * b + i] << (24 - 8 * (i % 4));
            sha::pad_block(w, len, b);
            sha::compress(h, w);
        }
        for (int i = 0; i < 8; i++) carried[i] = h[i];
    }
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(carried[i / 4] >> (24 - 8 * (i % 4)));
}

static int unhex(const std::string &s, std::vector<uint8_t> &out) {
    if (s.size() % 2) return -1;
    out.resize(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) {
        unsigned v;
        if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return -1;
        out[i] = (uint8_t)v;
    }
    return 0;
}

// The last blocks of a message of len bytes whose last len % 64 bytes are 0x5A, from an
// injected state: the tail builder's blocks against ones written out by hand with the bit
// count hi:lo, the two through the same rounds.
static int check_length_field(uint64_t len, uint32_t hi, uint32_t lo) {
    const uint32_t r = (uint32_t)(len % 64);
    const uint64_t first = len / 64, last = sha::blocks_of(len) - 1;
    CHECK(last == first + (r < 56 ? 0 : 1));
    uint8_t bytes[128] = {0};  // blocks `first` and, where there are two, `last`
    for (uint32_t i = 0; i < r; i++) bytes[i] = 0x5A;
    uint32_t h1[8], h2[8];
    for (int i = 0; i < 8; i++) h1[i] = h2[i] = (0x01234567u * (uint32_t)(i + 1)) ^ (uint32_t)len;  // the injected state
    for (uint64_t b = first; b <= last; b++) {
        uint32_t w[16] = {0};
        for (int i = 0; i < 64; i++) w[i / 4] |= (uint32_t)bytes[64 * (b - first) + i] << (24 - 8 * (i % 4));
        sha::pad_block(w, len, b);
        if (b == last) CHECK(w[14] == hi && w[15] == lo);
        sha::compress(h1, w);
    }
    bytes[r] = 0x80;
    uint8_t *end = bytes + 64 * (last - first + 1);
    for (int i = 0; i < 4; i++) end[-8 + i] = (uint8_t)(hi >> (24 - 8 * i)), end[-4 + i] = (uint8_t)(lo >> (24 - 8 * i));
    for (uint64_t b = first; b <= last; b++) {
        uint32_t want[16] = {0};
        for (int i = 0; i < 64; i++) want[i / 4] |= (uint32_t)bytes[64 * (b - first) + i] << (24 - 8 * (i % 4));
        sha::compress(h2, want);
    }
    for (int i = 0; i < 8; i++) CHECK(h1[i] == h2[i]);
    // and no earlier block of that message gets a length or a 0x80
    uint32_t z[16] = {0};
    sha::pad_block(z, len, first - 1);
    for (int i = 0; i < 16; i++) CHECK(z[i] == 0);
    return 0;
}

int main(int argc, char **argv) {
    // blocks per piece, padding included
    struct {
        uint64_t len, blocks;
    } t[] = {{0, 1}, {55, 1}, {56, 2}, {63, 2}, {64, 2}, {119, 2}, {120, 3}, {(1ull << 32) + 5, (1ull << 26) + 1},
             {kMaxLen, (1ull << 55) + 1}};
    for (auto &e : t) {
        CHECK(blocks_of(e.len) == e.blocks);
        CHECK(sha::blocks_of(e.len) == e.blocks);  // the kernel's own count
    }
    // fast / byte by alignment and run
    CHECK(class_of({4096, 100, 0, 0}) == kFast);
    CHECK(class_of({4096 + 16, 100, 0, 0}) == kFast);
    CHECK(class_of({4096 + 1, 100, 0, 0}) == kByte);
    CHECK(class_of({4096 + 8, 100000, 0, 0}) == kByte);
    CHECK(class_of({0, 0, 0, 0}) == kFast);                       // the empty piece at NULL
    CHECK(class_of({4096, 2048, 256, 29 * 256}) == kFast);        // RS(29,80) ess 256 data piece
    CHECK(class_of({4096 + 256, 2048, 256, 29 * 256}) == kFast);  // share 1
    CHECK(class_of({4096, 2048, 64, 4 * 64}) == kFast);           // 64-byte runs
    CHECK(class_of({4096, 2048, 32, 4 * 32}) == kByte);           // runs under 64 bytes
    CHECK(class_of({4096, 2048, 8, 32}) == kByte);
    CHECK(class_of({4096, 2400, 24, 72}) == kByte);               // no power of two
    CHECK(class_of({4096, 2048, 64, 72}) == kByte);               // a stride that breaks 16-byte alignment
    CHECK(class_of({4096, 2048, 2048, 99}) == kFast);             // one run: contiguous whatever the stride
    CHECK(class_of({4096, 1ull << 40, 0, 0}) == kFast);           // no oversize class
    // the lane order: ragged lengths, every third piece at an odd address, a strided piece; both orders
    std::vector<Piece> ps;
    uint64_t at = 1 << 20;
    for (uint64_t i = 0; i < 200; i++) {
        const uint64_t len = (37 * i) % 700 + (i == 78 ? 300000 : 0);
        ps.push_back({at + (i % 3 == 2 ? 1 : 0), len, 0, 0});
        at += (len + 64 + 15) / 16 * 16;
    }
    ps.push_back({at, 4096, 256, 29 * 256});
    ps.push_back({at, 4096, 8, 32});
    if (check_layout(ps)) return 1;
    std::vector<Piece> rev(ps.rbegin(), ps.rend());
    if (check_layout(rev)) return 1;
    if (check_layout({})) return 1;
    if (check_layout({{4096, 5, 0, 0}})) return 1;
    if (check_layout(std::vector<Piece>(kWave, Piece{4097, 5, 0, 0}))) return 1;      // one full byte wave, no fast wave
    if (check_layout(std::vector<Piece>(kWave + 1, Piece{4096, 5, 0, 0}))) return 1;  // one lane into a second wave
    {
        const Layout L = layout(ps.data(), ps.size());
        CHECK(L.count[kByte] == 66 + 1 && L.count[kFast] == 134 + 1);
        CHECK(L.waves() == 3 + 2);
        CHECK(ps[L.row[0]].len == 300000 + (37 * 78) % 700 && L.max_blocks == blocks_of(ps[L.row[0]].len));
    }
    // passes: at most kPassPieces pieces each
    std::vector<Pass> p = split(kPassPieces - 1);
    CHECK(p.size() == 1 && p[0].i0 == 0 && p[0].i1 == kPassPieces - 1);
    p = split(kPassPieces);
    CHECK(p.size() == 1 && p[0].i1 == kPassPieces);
    p = split(kPassPieces + 1);
    CHECK(p.size() == 2 && p[0].i1 == kPassPieces && p[1].i0 == kPassPieces && p[1].i1 == kPassPieces + 1);
    p = split(7, 3);
    CHECK(p.size() == 3 && p[0].i1 == 3 && p[1].i1 == 6 && p[2].i1 == 7);
    CHECK(split(0).empty());
    CHECK((uint64_t)kPassPieces + 2 * kWave < 1ull << 31);  // a pass's lane count fits 32 bits
    // launches
    CHECK(launches_of(0) == 0 && launches_of(1) == 1 && launches_of(kLaunchBlocks) == 1);
    CHECK(launches_of(kLaunchBlocks + 1) == 2);
    CHECK(launches_of(blocks_of(2314240)) == 3);  // an RS(29,80) piece of a 64 MiB segment: 36,161 blocks
    CHECK(launches_of(blocks_of(4096), 2) == 33 && launches_of(blocks_of(330), 2) == 3 && launches_of(1, 2) == 1);
    CHECK(launches_of(blocks_of(kMaxLen), 1) == (1ull << 55) + 1);
    // the kernel's rounds and tail builder on the given messages
    for (int a = 1; a < argc; a++) {
        const std::string s = argv[a];
        const size_t c1 = s.find(':'), c2 = s.rfind(':');
        CHECK(c1 != std::string::npos && c2 > c1);
        const uint64_t repeat = strtoull(s.substr(0, c1).c_str(), nullptr, 10);
        std::vector<uint8_t> unit, want, msg;
        CHECK(unhex(s.substr(c1 + 1, c2 - c1 - 1), unit) == 0 && unhex(s.substr(c2 + 1), want) == 0 && want.size() == 32);
        for (uint64_t i = 0; i < repeat; i++) msg.insert(msg.end(), unit.begin(), unit.end());
        for (uint64_t lb : {kLaunchBlocks, (uint64_t)1, (uint64_t)2, (uint64_t)1000}) {
            uint8_t got[32];
            hash_lane(msg.data(), msg.size(), lb, got);
            if (memcmp(got, want.data(), 32) != 0) {
                fprintf(stderr, "message %d (%zu bytes), %llu blocks per launch: digest differs\n", a, msg.size(),
                        (unsigned long long)lb);
                return 1;
            }
        }
    }
    // the bit count of lengths past 2^29 bytes (its high word), 2^32 bytes and at the limit
    if (check_length_field(1ull << 29, 1, 0)) return 1;
    if (check_length_field((1ull << 32) + 5, 8, 40)) return 1;
    if (check_length_field(kMaxLen, 0xFFFFFFFFu, 0xFFFFFFF8u)) return 1;
    puts("ok");
    return 0;
}
