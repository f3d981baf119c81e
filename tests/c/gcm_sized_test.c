/* Plain-C client of ec_gcm_seal_segments_sized and ec_gcm_open_segments_sized
 * (include/uplink_ec.h): the cgo view of the cipher of a batch of segments of
 * different sizes.  Three segments of three sizes through ec_device_alloc /
 * ec_copy, each under its own key and nonce: one seal, one open of the result,
 * and one open with a flipped tag bit.  Plaintexts, keys and nonces are a fixed
 * generator's bytes; the expected ciphertexts come from the test that runs this
 * program (the CPU oracle's), as hexadecimal arguments, one per segment.  Built
 * and run by tests/test_gcm_sized_c.py. */
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

/* byte i of segment g's plaintext, key and nonce (the test generates the same) */
static uint8_t seg_byte(int g, size_t i) { return (uint8_t)((i * 2654435761u + (size_t)g * 40503u) >> 11); }
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
    static const size_t nblocks[NSEG] = {1, 3, 4}; /* a wave, a wave short of a workgroup, a full workgroup */
    uint8_t *want[NSEG];
    if (argc != 1 + NSEG) {
        fprintf(stderr, "usage: gcm_sized_test <ciphertext of segment 0, hex> <1> <2>\n");
        return 2;
    }
    for (int g = 0; g < NSEG; g++) {
        want[g] = malloc(nblocks[g] * OUT_BLOCK);
        if (unhex(argv[1 + g], want[g], nblocks[g] * OUT_BLOCK)) {
            fprintf(stderr, "argument %d is not %zu bytes of hex\n", 1 + g, nblocks[g] * OUT_BLOCK);
            return 2;
        }
    }
    ec_ctx *ctx = NULL;
    int rc = ec_create(29, 80, 256, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    /* keys and nonces */
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
    /* per segment: plaintext, and a ciphertext and an opened buffer between guards of 0xCD */
    uint8_t *plain[NSEG], *d_plain[NSEG], *d_enc[NSEG], *d_back[NSEG], *enc_out[NSEG], *back_out[NSEG];
    const uint8_t *enc_in[NSEG];
    for (int g = 0; g < NSEG; g++) {
        const size_t pb = nblocks[g] * IN_BLOCK, eb = nblocks[g] * OUT_BLOCK;
        plain[g] = malloc(pb);
        for (size_t i = 0; i < pb; i++) plain[g][i] = seg_byte(g, i);
        uint8_t *blank = malloc(eb + 2 * GUARD);
        memset(blank, 0xCD, eb + 2 * GUARD);
        d_plain[g] = ec_device_alloc(pb);
        d_enc[g] = ec_device_alloc(eb + 2 * GUARD);
        d_back[g] = ec_device_alloc(pb + 2 * GUARD);
        CHECK(d_plain[g] && d_enc[g] && d_back[g], "ec_device_alloc");
        if (!d_plain[g] || !d_enc[g] || !d_back[g]) return 1;
        CHECK(ec_copy(d_plain[g], plain[g], pb) == EC_OK, "ec_copy H2D");
        CHECK(ec_copy(d_enc[g], blank, eb + 2 * GUARD) == EC_OK && ec_copy(d_back[g], blank, pb + 2 * GUARD) == EC_OK,
              "fill");
        free(blank);
        enc_in[g] = enc_out[g] = d_enc[g] + GUARD;
        back_out[g] = d_back[g] + GUARD;
    }
    /* a segment without its output: refused, nothing written */
    uint8_t *out_bad[NSEG] = {enc_out[0], NULL, enc_out[2]};
    rc = ec_gcm_seal_segments_sized(ctx, NSEG, d_plain, nblocks, NULL, IN_BLOCK, d_keys, d_nonces, out_bad, NULL);
    CHECK(rc == EC_ERR_INVALID_ARG, "a NULL out[1]: rc %d", rc);
    rc = ec_gcm_seal_segments_sized(ctx, NSEG, d_plain, nblocks, NULL, IN_BLOCK, d_keys, d_nonces, enc_out, NULL);
    CHECK(rc == EC_OK, "ec_gcm_seal_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    for (int g = 0; g < NSEG; g++) {
        const size_t eb = nblocks[g] * OUT_BLOCK;
        uint8_t *got = malloc(eb + 2 * GUARD);
        CHECK(ec_copy(got, d_enc[g], eb + 2 * GUARD) == EC_OK, "ec_copy D2H"); /* (waits for the default stream) */
        CHECK(memcmp(got + GUARD, want[g], eb) == 0, "segment %d: ciphertext differs", g);
        for (int i = 0; i < GUARD; i++)
            CHECK(got[i] == 0xCD && got[GUARD + eb + i] == 0xCD, "segment %d: a guard of the ciphertext was written", g);
        free(got);
    }
    int32_t status[NSEG] = {7, 7, 7};
    rc = ec_gcm_open_segments_sized(ctx, NSEG, enc_in, nblocks, IN_BLOCK, d_keys, d_nonces, back_out, d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status");
    for (int g = 0; g < NSEG; g++) {
        const size_t pb = nblocks[g] * IN_BLOCK;
        uint8_t *got = malloc(pb + 2 * GUARD);
        CHECK(status[g] == -1, "segment %d: status %d", g, (int)status[g]);
        CHECK(ec_copy(got, d_back[g], pb + 2 * GUARD) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(got + GUARD, plain[g], pb) == 0, "segment %d: plaintext differs", g);
        for (int i = 0; i < GUARD; i++)
            CHECK(got[i] == 0xCD && got[GUARD + pb + i] == 0xCD, "segment %d: a guard of the plaintext was written", g);
        free(got);
    }
    /* a tag bit of block 2 of segment 1 */
    uint8_t tagbyte = want[1][2 * OUT_BLOCK + IN_BLOCK + 5] ^ 0x20;
    CHECK(ec_copy(d_enc[1] + GUARD + 2 * OUT_BLOCK + IN_BLOCK + 5, &tagbyte, 1) == EC_OK, "ec_copy tag");
    rc = ec_gcm_open_segments_sized(ctx, NSEG, enc_in, nblocks, IN_BLOCK, d_keys, d_nonces, back_out, d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status");
    CHECK(status[0] == -1 && status[1] == 2 && status[2] == -1, "status %d %d %d after a flipped tag bit", (int)status[0],
          (int)status[1], (int)status[2]);
    unsigned long long seals = 0, opens = 0, passes = 0;
    CHECK(ec_gcm_sized_stats(ctx, &seals, &opens, &passes) == EC_OK, "ec_gcm_sized_stats");
    CHECK(seals == 1 && opens == 2 && passes == 3, "launches %llu %llu %llu", seals, opens, passes);
    for (int g = 0; g < NSEG; g++) {
        ec_device_free(d_plain[g]);
        ec_device_free(d_enc[g]);
        ec_device_free(d_back[g]);
        free(plain[g]);
        free(want[g]);
    }
    ec_device_free(d_keys);
    ec_device_free(d_nonces);
    ec_device_free(d_status);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: %d segments of %zu, %zu and %zu blocks sealed and opened in one call each\n", NSEG, nblocks[0],
           nblocks[1], nblocks[2]);
    return 0;
}
