// The arithmetic of the one-shot message cipher on the host
// (uplink_amd/csrc/gcm_msg_device.hpp, the code the kernel gcm_messages runs;
// lane geometry from gcm_msg_geom.hpp): a stand-alone program that plays the 64
// lanes of a message's wave in a loop -- key expansion from the 32 key bytes, H
// and AES_K(J0), every lane's Horner run over its consecutive slots, H^rounds run
// up beside it, the pairwise combination of the 64 partial sums -- and seals and
// opens messages given as hex, once with each form of the multiply.
//
//   gcm_msg_host_test FILE      FILE: lines of "key nonce plain sealed" in hex, "-" for empty
//
// Every line must seal to exactly `sealed` and open back to `plain`; a flipped
// tag bit, ciphertext bit (when there is one) and key bit must fail to open.
// Prints "ok <lines>".  Built by tests/test_messages_host.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gcm_msg_device.hpp"
#include "gcm_msg_geom.hpp"

using namespace uplink_ec::gcmmsg;

namespace {

// the AES S-box from its definition: the inverse in GF(2^8) mod 0x11b, then the affine map
struct SboxTable {
    uint8_t s[256];
    SboxTable() {
        uint8_t ex[256] = {}, lg[256] = {};
        uint8_t p = 1;
        for (int i = 0; i < 255; i++) {
            ex[i] = p;
            lg[p] = (uint8_t)i;
            p = (uint8_t)(p ^ (uint8_t)((p << 1) ^ ((p & 0x80) ? 0x1b : 0)));  // times the generator 3
        }
        for (int x = 0; x < 256; x++) {
            const uint8_t inv = x ? ex[(255 - lg[x]) % 255] : 0;
            uint8_t v = inv, r = inv;
            for (int i = 0; i < 4; i++) {
                r = (uint8_t)((r << 1) | (r >> 7));
                v ^= r;
            }
            s[x] = (uint8_t)(v ^ 0x63);
        }
    }
};
const SboxTable kSbox;
struct Sbox {
    uint32_t operator()(uint32_t x) const { return kSbox.s[x & 255]; }
};

int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "line %d: %s failed\n", __LINE__, #c);  \
            failures++;                                             \
        }                                                           \
    } while (0)

std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

// What one wave does for one message.  open: `in` is ciphertext || tag; returns false when the tag
// does not verify (out is then zeros).  Otherwise `in` is the plaintext and out ciphertext || tag.
template <class Mul>
bool message(const uint8_t key[32], const uint8_t nonce[12], const std::vector<uint8_t> &in, bool open,
             std::vector<uint8_t> &out) {
    const uint64_t len = open ? in.size() - kTagBytes : in.size();
    uint32_t kw[8], rk[60], nw[3];
    for (int i = 0; i < 8; i++) kw[i] = load_be32(key + 4 * i);
    for (int i = 0; i < 3; i++) nw[i] = load_be32(nonce + 4 * i);
    key_expand(kw, rk, Sbox());
    const Block h = aes256_encrypt(zero_block(), rk, Sbox());
    const Block ekj0 = aes256_encrypt(counter_block(nw, 1), rk, Sbox());
    const uint32_t R = rounds(len), pad = front_pad(len), nd = data_slots(len), tail = tail_bytes(len);
    out.assign(open ? len : len + kTagBytes, 0);
    Mul mul;
    mul.set(h);
    Block partial[64], hr = h;
    for (uint32_t lane = 0; lane < kLanes; lane++) {
        Block acc = zero_block();
        for (uint32_t j = 0; j < R; j++) {
            const uint32_t t = lane * R + j;
            Block y = zero_block();
            if (slot_kind(len, t) == Slot::kData) {
                const uint32_t sidx = t - pad, n = sidx + 1 == nd ? tail : 16;
                const Block x = load_bytes(in.data() + 16 * (size_t)sidx, n);
                if (open) {
                    y = x;
                } else {
                    const Block o = x ^ aes256_encrypt(counter_block(nw, 2 + sidx), rk, Sbox());
                    for (uint32_t i = 0; i < n; i++) out[16 * (size_t)sidx + i] = block_byte(o, i);
                    y = keep_bytes(o, n);
                }
            } else if (slot_kind(len, t) == Slot::kLength) {
                CHECK(lane == 63 && j + 1 == R);
                y = length_block(len);
            }
            acc = horner_step(acc, y, mul);
            if (lane == 0 && j) hr = mul.mul(hr);  // (the same in every lane)
        }
        partial[lane] = acc;
        if (lane + live_lanes(len) < kLanes) CHECK(acc == zero_block());
    }
    const Block tag = combine64(partial, hr, combine_steps(len), mul) ^ ekj0;
    if (!open) {
        for (uint32_t i = 0; i < 16; i++) out[len + i] = block_byte(tag, i);
        return true;
    }
    bool ok = true;
    for (uint32_t i = 0; i < 16; i++) ok &= in[len + i] == block_byte(tag, i);
    if (!ok) return false;
    for (uint32_t sidx = 0; sidx < nd; sidx++) {
        const uint32_t n = sidx + 1 == nd ? tail : 16;
        const Block o = load_bytes(in.data() + 16 * (size_t)sidx, n) ^ aes256_encrypt(counter_block(nw, 2 + sidx), rk, Sbox());
        for (uint32_t i = 0; i < n; i++) out[16 * (size_t)sidx + i] = block_byte(o, i);
    }
    return true;
}

template <class Mul>
void run_line(const std::vector<uint8_t> &key, const std::vector<uint8_t> &nonce, const std::vector<uint8_t> &plain,
              const std::vector<uint8_t> &sealed) {
    std::vector<uint8_t> out;
    CHECK(message<Mul>(key.data(), nonce.data(), plain, false, out));
    CHECK(out == sealed);
    CHECK(message<Mul>(key.data(), nonce.data(), sealed, true, out));
    CHECK(out == plain);
    std::vector<uint8_t> bad = sealed;
    bad[bad.size() - 1] ^= 0x01;
    CHECK(!message<Mul>(key.data(), nonce.data(), bad, true, out));
    CHECK(out == std::vector<uint8_t>(plain.size(), 0));
    if (!plain.empty()) {
        bad = sealed;
        bad[0] ^= 0x80;
        CHECK(!message<Mul>(key.data(), nonce.data(), bad, true, out));
        bad = sealed;
        bad[plain.size() - 1] ^= 0x01;
        CHECK(!message<Mul>(key.data(), nonce.data(), bad, true, out));
    }
    std::vector<uint8_t> k2 = key;
    k2[31] ^= 0x01;
    CHECK(!message<Mul>(k2.data(), nonce.data(), sealed, true, out));
}

// the two multiplies and the table's parts against each other and against the field's axioms
void field_checks() {
    Block a{{0x66e94bd4u, 0xef8a2c3bu, 0x884cfa59u, 0xca342b2eu}}, b{{0x0388daceu, 0x60b6a392u, 0xf328c2b9u, 0x71b2fe78u}};
    const Block one{{0x80000000u, 0, 0, 0}};
    for (int it = 0; it < 64; it++) {
        MulTable t;
        t.set(b);
        const Block p = gf_mul_bits(a, b);
        CHECK(p == gf_mul_bits(b, a));
        CHECK(p == t.mul(a));
        CHECK(gf_mul_bits(a, one) == a);
        CHECK(gf_times_x(a) == gf_mul_bits(a, Block{{0x40000000u, 0, 0, 0}}));
        for (uint32_t n = 0; n < 16; n++) CHECK(t.tab[n] == gf_mul_bits(Block{{n << 28, 0, 0, 0}}, b));
        a = p ^ Block{{(uint32_t)it, 0, 0, 1}};
        b = gf_times_x(b ^ a);
    }
    // the specification's test case 2 intermediate: H * (C1) ... checked through the vectors below
    for (uint32_t n = 0; n < 16; n++) {
        uint32_t want = 0;
        for (int bit = 0; bit < 4; bit++)
            if (n & (1u << bit)) want ^= 0x1C20u << bit;
        CHECK(gf_rem4(n) == want << 16);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: gcm_msg_host_test FILE\n");
        return 2;
    }
    field_checks();
    std::ifstream fh(argv[1]);
    std::string line;
    int lines = 0;
    while (std::getline(fh, line)) {
        std::istringstream is(line);
        std::string k, n, p, s;
        if (!(is >> k >> n >> p >> s)) continue;
        const auto key = unhex(k), nonce = unhex(n), plain = unhex(p), sealed = unhex(s);
        if (key.size() != 32 || nonce.size() != 12 || sealed.size() != plain.size() + 16) {
            fprintf(stderr, "malformed line %d\n", lines + 1);
            return 2;
        }
        const int before = failures;
        run_line<MulBits>(key, nonce, plain, sealed);
        run_line<MulTable>(key, nonce, plain, sealed);
        if (failures != before) fprintf(stderr, "  (message %d, %zu bytes)\n", lines, plain.size());
        lines++;
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ok %d\n", lines);
    return 0;
}
