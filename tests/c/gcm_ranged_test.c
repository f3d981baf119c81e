/* Plain-C client of ec_gcm_open_ranges_sized (include/uplink_ec.h): the cgo view
 * of a batch of ranged downloads.  Three ranges through ec_device_alloc /
 * ec_copy, each of its own segment, key, nonce and first block: two whole
 * blocks at 16-byte aligned addresses, 10,000 bytes that start 6,608 bytes into
 * block 3 with source and output at odd addresses, and one byte.  Keys and
 * nonces are a fixed generator's bytes; the covered blocks' ciphertext and the
 * expected plaintext of each range come from the test that runs this program
 * (the CPU oracle's), as hexadecimal arguments: ciphertext 0, plaintext 0,
 * ciphertext 1, ...  Built and run by tests/test_ranges_c.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uplink_ec.h"

static int failures = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            failures++;                               \
            fprintf(stderr, "FAIL: " __VA_ARGS__);    \
            fprintf(stderr, "\n");                    \
        }                                             \
    } while (0)

enum { NSEG = 3, IN_BLOCK = 7408, OUT_BLOCK = IN_BLOCK + 16, GUARD = 64 };

/* (as tests/test_ranges_c.py has them) */
static const size_t first_block[NSEG] = {0, 3, 1};
static const size_t nblocks[NSEG] = {2, 3, 1};
static const size_t head[NSEG] = {0, 6608, 17};
static const size_t length[NSEG] = {2 * IN_BLOCK, 10000, 1};
static const size_t in_shift[NSEG] = {0, 1, 8}, out_shift[NSEG] = {0, 15, 3}; /* bytes past a 16-byte boundary */

static uint8_t key_byte(int g, int i) { return (uint8_t)(g * 37 + i * 11 + 5); }
static uint8_t nonce_byte(int g, int i) { return (uint8_t)(g * 101 + i * 7 + 250); }

static int unhex(const char *s, uint8_t *out, size_t n) {
    if (strlen(s) != 2 * n) return -1;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return -1;
        out[i] = (uint8_t)v;
    }
    return 0;
}

int main(int argc, char **argv) {
    uint8_t *enc[NSEG], *want[NSEG];
    if (argc != 1 + 2 * NSEG) {
        fprintf(stderr, "usage: gcm_ranged_test <covered blocks of range 0, hex> <its plaintext, hex> <1> <1> <2> <2>\n");
        return 2;
    }
    for (int g = 0; g < NSEG; g++) {
        enc[g] = malloc(nblocks[g] * OUT_BLOCK);
        want[g] = malloc(length[g]);
        if (unhex(argv[1 + 2 * g], enc[g], nblocks[g] * OUT_BLOCK) || unhex(argv[2 + 2 * g], want[g], length[g])) {
            fprintf(stderr, "the arguments of range %d are not %zu and %zu bytes of hex\n", g, nblocks[g] * OUT_BLOCK,
                    length[g]);
            return 2;
        }
    }
    ec_ctx *ctx = NULL;
    int rc = ec_create(29, 80, 256, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t keys[NSEG * 32], nonces[NSEG * 12];
    for (int g = 0; g < NSEG; g++) {
        for (int i = 0; i < 32; i++) keys[32 * g + i] = key_byte(g, i);
        for (int i = 0; i < 12; i++) nonces[12 * g + i] = nonce_byte(g, i);
    }
    void *d_keys = ec_device_alloc(NSEG * ec_gcm_key_bytes());
    uint8_t *d_nonces = ec_device_alloc(sizeof nonces);
    int32_t *d_status = ec_device_alloc(NSEG * sizeof(int32_t));
    CHECK(d_keys && d_nonces && d_status, "ec_device_alloc");
    if (!d_keys || !d_nonces || !d_status) return 1;
    rc = ec_gcm_prepare_keys(keys, NSEG, d_keys, NULL);
    CHECK(rc == EC_OK, "ec_gcm_prepare_keys rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(d_nonces, nonces, sizeof nonces) == EC_OK, "ec_copy nonces");
    /* per range: its covered blocks and its output, each between guards of 0xCD, shifted off 16-byte alignment */
    uint8_t *d_enc[NSEG], *d_out[NSEG], *out[NSEG];
    const uint8_t *in[NSEG];
    for (int g = 0; g < NSEG; g++) {
        const size_t eb = nblocks[g] * OUT_BLOCK, ecap = eb + 2 * GUARD + 16, ocap = length[g] + 2 * GUARD + 16;
        uint8_t *blank = malloc(ecap > ocap ? ecap : ocap);
        memset(blank, 0xCD, ecap > ocap ? ecap : ocap);
        d_enc[g] = ec_device_alloc(ecap);
        d_out[g] = ec_device_alloc(ocap);
        CHECK(d_enc[g] && d_out[g], "ec_device_alloc");
        if (!d_enc[g] || !d_out[g]) return 1;
        CHECK(((uintptr_t)d_enc[g] & 15) == 0 && ((uintptr_t)d_out[g] & 15) == 0, "device allocations are 16-byte aligned");
        CHECK(ec_copy(d_enc[g], blank, ecap) == EC_OK && ec_copy(d_out[g], blank, ocap) == EC_OK, "fill");
        free(blank);
        in[g] = d_enc[g] + GUARD + in_shift[g];
        out[g] = d_out[g] + GUARD + out_shift[g];
        CHECK(ec_copy(d_enc[g] + GUARD + in_shift[g], enc[g], eb) == EC_OK, "ec_copy H2D");
    }
    /* a block count that does not cover its range: refused, nothing written */
    size_t nb_bad[NSEG] = {nblocks[0], nblocks[1] - 1, nblocks[2]};
    rc = ec_gcm_open_ranges_sized(ctx, NSEG, in, first_block, nb_bad, head, length, IN_BLOCK, d_keys, d_nonces, out,
                                  d_status, NULL);
    CHECK(rc == EC_ERR_INVALID_ARG, "2 blocks for a range over 3: rc %d", rc);
    int32_t status[NSEG] = {7, 7, 7};
    rc = ec_gcm_open_ranges_sized(ctx, NSEG, in, first_block, nblocks, head, length, IN_BLOCK, d_keys, d_nonces, out,
                                  d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_ranges_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status"); /* (waits for the default stream) */
    for (int g = 0; g < NSEG; g++) {
        const size_t cap = length[g] + 2 * GUARD + 16, at = GUARD + out_shift[g];
        uint8_t *got = malloc(cap);
        CHECK(status[g] == -1, "range %d: status %d", g, (int)status[g]);
        CHECK(ec_copy(got, d_out[g], cap) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(got + at, want[g], length[g]) == 0, "range %d: plaintext differs", g);
        for (size_t i = 0; i < cap; i++)
            if (i < at || i >= at + length[g]) CHECK(got[i] == 0xCD, "range %d: byte %zu outside its output was written", g, i);
        free(got);
    }
    /* a ciphertext bit of block 2 of range 1 (absolute block 5), behind the bytes the range wants */
    uint8_t flipped = enc[1][2 * OUT_BLOCK + 4000] ^ 0x20;
    CHECK((head[1] + length[1]) % IN_BLOCK < 4000, "byte 4000 of the last block is outside the range");
    CHECK(ec_copy(d_enc[1] + GUARD + in_shift[1] + 2 * OUT_BLOCK + 4000, &flipped, 1) == EC_OK, "ec_copy bit");
    rc = ec_gcm_open_ranges_sized(ctx, NSEG, in, first_block, nblocks, head, length, IN_BLOCK, d_keys, d_nonces, out,
                                  d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_ranges_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status");
    CHECK(status[0] == -1 && status[1] == 5 && status[2] == -1, "status %d %d %d after a flipped bit", (int)status[0],
          (int)status[1], (int)status[2]);
    unsigned long long opens = 0, passes = 0, s_seal = 9, s_open = 9, s_passes = 9;
    CHECK(ec_gcm_ranged_stats(ctx, &opens, &passes) == EC_OK, "ec_gcm_ranged_stats");
    CHECK(opens == 2 && passes == 2, "launches %llu, passes %llu", opens, passes);
    CHECK(ec_gcm_sized_stats(ctx, &s_seal, &s_open, &s_passes) == EC_OK && s_seal == 0 && s_open == 0 && s_passes == 0,
          "the sized calls' counters moved");
    for (int g = 0; g < NSEG; g++) {
        ec_device_free(d_enc[g]);
        ec_device_free(d_out[g]);
        free(enc[g]);
        free(want[g]);
    }
    ec_device_free(d_keys);
    ec_device_free(d_nonces);
    ec_device_free(d_status);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: %d ranges of %zu, %zu and %zu bytes opened in one call\n", NSEG, length[0], length[1], length[2]);
    return 0;
}
