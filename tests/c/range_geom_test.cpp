// Stand-alone program over uplink_amd/csrc/range_geom.hpp (no HIP): the geometry
// of a ranged download against a definitional model -- mark the wanted plaintext
// bytes, the cipher blocks that hold any, the encrypted bytes of those blocks and
// the stripes that hold any -- for EVERY (offset, length) of several plaintext
// sizes at small blocks and stripes; the geometry must be exactly that minimal
// cover, with head and skip as defined.  Then the worked example of RS(29,80),
// the overflow and 0x7FFFFFFF edges, and the rule ec_gcm_open_ranges_sized puts
// on (head, length, nblocks).  Built with the host compiler under
// -fsanitize=address,undefined by tests/test_ranges_host.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "range_geom.hpp"

using namespace uplink_ec::rangegeom;

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// first and count of the set entries of m, which must be one run (count 0: none set)
static bool run_of(const std::vector<uint8_t> &m, uint64_t *first, uint64_t *count) {
    uint64_t lo = m.size(), hi = 0, n = 0;
    for (uint64_t i = 0; i < m.size(); i++)
        if (m[i]) {
            if (i < lo) lo = i;
            hi = i;
            n++;
        }
    *first = n ? lo : 0;
    *count = n;
    return n == 0 || hi - lo + 1 == n;
}

static int check_all(uint64_t P, uint64_t ib, uint64_t k, uint64_t ess) {
    const uint64_t B = ib + 16, S = k * ess;
    const uint64_t nblk = P / ib + 1, enc = nblk * B, nstr = enc / S + 1;
    for (uint64_t off = 0; off <= P; off++)
        for (uint64_t len = 0; off + len <= P; len++) {
            const RangeGeom g = range_geometry(P, off, len, B, k, ess);
            CHECK(g.err == kOk);
            // the model
            std::vector<uint8_t> blocks(nblk, 0), ebytes(enc, 0), stripes(nstr, 0);
            for (uint64_t p = off; p < off + len; p++) blocks[p / ib] = 1;
            for (uint64_t b = 0; b < nblk; b++)
                if (blocks[b])
                    for (uint64_t e = b * B; e < (b + 1) * B; e++) ebytes[e] = 1;
            for (uint64_t e = 0; e < enc; e++)
                if (ebytes[e]) stripes[e / S] = 1;
            uint64_t fb, nb, fs, ns;
            CHECK(run_of(blocks, &fb, &nb) && run_of(stripes, &fs, &ns));
            CHECK(g.nblocks == nb && g.nstripes == ns);
            if (len == 0) {  // no block, no stripe; the first ones are where the offset lies
                CHECK(nb == 0 && ns == 0);
                fb = off / ib;
                fs = fb * B / S;
            }
            CHECK(g.first_block == fb && g.head == off - fb * ib && g.head < ib);
            CHECK(g.enc_off == fb * B && g.enc_len == nb * B);
            CHECK(g.first_stripe == fs && g.skip == fb * B - fs * S && g.skip < S);
            CHECK(g.piece_off == fs * ess && g.piece_len == ns * ess);
            // the covered blocks lie inside the decoded stripes, the range inside the covered blocks
            CHECK(g.skip + g.enc_len <= ns * S || nb == 0);
            CHECK(g.head + len <= nb * ib || nb == 0);
            CHECK(covers(g.head, len, ib, nb));
            CHECK(!covers(g.head, len, ib, nb + 1) && (nb == 0 || !covers(g.head, len, ib, nb - 1)));
            // it is encryption.CalcEncompassingBlocks twice
            const Blocks cb = encompassing_blocks(off, len, ib), cs = encompassing_blocks(cb.first * B, cb.count * B, S);
            CHECK(cb.first == g.first_block && cb.count == nb && cs.first == g.first_stripe && cs.count == ns);
        }
    return 0;
}

int main() {
    const uint64_t schemes[3][2] = {{2, 8}, {3, 8}, {4, 16}};  // (k, ess)
    for (uint64_t ib : {16u, 32u, 48u})
        for (auto &ke : schemes)
            for (uint64_t P : {0u, 1u, 47u, 96u, 160u})
                if (check_all(P, ib, ke[0], ke[1])) return 1;
    // RS(29,80), ess 256, block 7424: 1 MiB at 10,000,000 of a 64 MiB segment
    {
        const RangeGeom g = range_geometry(67108864, 10000000, 1048576, 7424, 29, 256);
        CHECK(g.err == kOk && g.first_block == 1349 && g.head == 6608 && g.nblocks == 143);
        CHECK(g.enc_off == 10014976 && g.enc_len == 143 * 7424);
        CHECK(g.first_stripe == 1349 && g.nstripes == 143 && g.skip == 0);
        CHECK(g.piece_off == 345344 && g.piece_len == 36608);
        CHECK(29 * g.piece_len == 1061632);  // piece bytes in for 1,048,576 plaintext bytes out
    }
    // RS(3,7), ess 8, block 32: skip cycles through 0, 8, 16
    for (uint64_t fb = 0; fb < 6; fb++) {
        const RangeGeom g = range_geometry(1000, fb * 16, 16, 32, 3, 8);
        CHECK(g.err == kOk && g.first_block == fb && g.skip == (fb * 32) % 24 && g.skip % 8 == 0);
    }
    // outside [0, P], overflow, shapes
    CHECK(range_geometry(100, 101, 0, 32, 2, 8).err == kInvalid);
    CHECK(range_geometry(100, 100, 0, 32, 2, 8).err == kOk);
    CHECK(range_geometry(100, 50, 51, 32, 2, 8).err == kInvalid);
    CHECK(range_geometry(UINT64_MAX, UINT64_MAX - 5, 10, 32, 2, 8).err == kInvalid);  // off + len wraps
    CHECK(range_geometry(100, 0, 1, 16, 2, 8).err == kInvalid);                       // no plaintext in a block
    CHECK(range_geometry(100, 0, 1, 40, 2, 8).err == kInvalid);                       // in_block 24
    CHECK(range_geometry(100, 0, 1, (1u << 24) + 32, 2, 8).err == kInvalid);          // in_block above 1<<24
    CHECK(range_geometry(100, 0, 1, (1u << 24) + 16, 2, 8).err == kOk);
    CHECK(range_geometry(100, 0, 1, 32, 0, 8).err == kInvalid && range_geometry(100, 0, 1, 32, 2, 0).err == kInvalid);
    CHECK(range_geometry(100, 0, 1, 32, 1ull << 40, 1ull << 40).err == kInvalid);  // k * ess wraps
    {
        const RangeGeom z = range_geometry(100, 101, 0, 32, 2, 8);  // an error leaves zeros
        CHECK(z.first_block == 0 && z.nblocks == 0 && z.enc_len == 0 && z.nstripes == 0 && z.piece_len == 0);
    }
    // first block + blocks at 0x7FFFFFFF and one over (status words are int32)
    {
        const uint64_t top = 0x7FFFFFFFull * 16;  // the end of block 0x7FFFFFFE at in_block 16
        RangeGeom g = range_geometry(top + 16, top - 16, 16, 32, 2, 8);
        CHECK(g.err == kOk && g.first_block == 0x7FFFFFFEu && g.nblocks == 1);
        g = range_geometry(top + 16, top - 16, 17, 32, 2, 8);
        CHECK(g.err == kUnsupported && g.nblocks == 0);
        g = range_geometry(top + 16, top, 1, 32, 2, 8);
        CHECK(g.err == kUnsupported);
        g = range_geometry(top + 16, 0, top, 32, 2, 8);
        CHECK(g.err == kOk && g.nblocks == 0x7FFFFFFFu && g.enc_len == 0x7FFFFFFFull * 32);
        g = range_geometry(top + 16, 0, top + 1, 32, 2, 8);
        CHECK(g.err == kUnsupported);
    }
    // the call's rule on (head, length, nblocks)
    CHECK(covers(0, 0, 16, 0) && covers(15, 0, 16, 0) && !covers(16, 0, 16, 0) && !covers(0, 0, 0, 0));
    CHECK(covers(0, 16, 16, 1) && covers(1, 16, 16, 2) && covers(15, 1, 16, 1) && covers(15, 2, 16, 2));
    CHECK(!covers(0, 1, 16, 0) && !covers(0, 0, 16, 1) && !covers(0, 17, 16, 1));
    CHECK(!covers(5, UINT64_MAX, 16, 1) && !covers(5, UINT64_MAX - 4, 16, 1));
    puts("ok");
    return 0;
}
