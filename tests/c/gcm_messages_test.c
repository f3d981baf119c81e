/* Plain-C client of ec_gcm_seal_messages / ec_gcm_open_messages
 * (include/uplink_ec.h): the cgo view of a batch of one-shot messages, a raw
 * 32-byte key each and no prepared keys.  Three messages through
 * ec_device_alloc / ec_copy: 100 bytes at 16-byte aligned addresses, 32 bytes (a
 * content key) with source and output at odd addresses, and an empty one.  They
 * are sealed in one call and compared with the sealed bytes the test that runs
 * this program hands in (the CPU oracle's), as hexadecimal arguments: plaintext
 * 0, sealed 0, plaintext 1, ... ("-" for no bytes); then opened in one call,
 * then opened again with a tag bit of message 1 flipped.  Keys and nonces are a
 * fixed generator's bytes.  Built and run by tests/test_messages_c.py. */
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

enum { NMSG = 3, TAG = 16, GUARD = 64 };

/* (as tests/test_messages_c.py has them) */
static const size_t len[NMSG] = {100, 32, 0};
static const size_t in_shift[NMSG] = {0, 1, 8}, out_shift[NMSG] = {0, 15, 3}; /* bytes past a 16-byte boundary */

static uint8_t key_byte(int g, int i) { return (uint8_t)(g * 37 + i * 11 + 5); }
static uint8_t nonce_byte(int g, int i) { return (uint8_t)(g * 101 + i * 7 + 250); }

static int unhex(const char *s, uint8_t *out, size_t n) {
    if (n == 0) return strcmp(s, "-") ? -1 : 0;
    if (strlen(s) != 2 * n) return -1;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return -1;
        out[i] = (uint8_t)v;
    }
    return 0;
}

/* a device window of n bytes, `shift` past a 16-byte boundary, between guards of 0xCD */
static uint8_t *window(size_t n, size_t shift, uint8_t **base, size_t *cap) {
    *cap = n + 2 * GUARD + 16;
    uint8_t *blank = malloc(*cap);
    memset(blank, 0xCD, *cap);
    *base = ec_device_alloc(*cap);
    CHECK(*base && ((uintptr_t)*base & 15) == 0, "ec_device_alloc");
    if (!*base) exit(1);
    CHECK(ec_copy(*base, blank, *cap) == EC_OK, "fill");
    free(blank);
    return *base + GUARD + shift;
}

/* the window holds want[0..n) and 0xCD everywhere else */
static void check_window(const char *what, int g, uint8_t *base, size_t cap, size_t shift, const uint8_t *want, size_t n) {
    uint8_t *got = malloc(cap);
    const size_t at = GUARD + shift;
    CHECK(ec_copy(got, base, cap) == EC_OK, "ec_copy D2H");
    CHECK(n == 0 || memcmp(got + at, want, n) == 0, "%s %d differs", what, g);
    for (size_t i = 0; i < cap; i++)
        if (i < at || i >= at + n) CHECK(got[i] == 0xCD, "%s %d: byte %zu outside it was written", what, g, i);
    free(got);
}

int main(int argc, char **argv) {
    uint8_t *plain[NMSG], *sealed[NMSG];
    if (argc != 1 + 2 * NMSG) {
        fprintf(stderr, "usage: gcm_messages_test <plaintext 0, hex> <sealed 0, hex> <1> <1> <2> <2>\n");
        return 2;
    }
    for (int g = 0; g < NMSG; g++) {
        plain[g] = malloc(len[g] + 1);
        sealed[g] = malloc(len[g] + TAG);
        if (unhex(argv[1 + 2 * g], plain[g], len[g]) || unhex(argv[2 + 2 * g], sealed[g], len[g] + TAG)) {
            fprintf(stderr, "the arguments of message %d are not %zu and %zu bytes of hex\n", g, len[g], len[g] + TAG);
            return 2;
        }
    }
    ec_ctx *ctx = NULL;
    int rc = ec_create(29, 80, 256, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t keys[NMSG * 32], nonces[NMSG * 12];
    for (int g = 0; g < NMSG; g++) {
        for (int i = 0; i < 32; i++) keys[32 * g + i] = key_byte(g, i);
        for (int i = 0; i < 12; i++) nonces[12 * g + i] = nonce_byte(g, i);
    }
    /* raw key bytes and nonces in device memory, both at odd addresses */
    uint8_t *d_kn = ec_device_alloc(sizeof keys + sizeof nonces + 16);
    int32_t *d_status = ec_device_alloc(NMSG * sizeof(int32_t));
    CHECK(d_kn && d_status, "ec_device_alloc");
    if (!d_kn || !d_status) return 1;
    uint8_t *d_keys = d_kn + 3, *d_nonces = d_kn + 3 + sizeof keys;
    CHECK(ec_copy(d_keys, keys, sizeof keys) == EC_OK && ec_copy(d_nonces, nonces, sizeof nonces) == EC_OK, "ec_copy");

    uint8_t *b_plain[NMSG], *b_sealed[NMSG], *b_back[NMSG], *out[NMSG], *back[NMSG];
    const uint8_t *in[NMSG], *cin[NMSG];
    size_t c_plain[NMSG], c_sealed[NMSG], c_back[NMSG];
    for (int g = 0; g < NMSG; g++) {
        uint8_t *p = window(len[g], in_shift[g], &b_plain[g], &c_plain[g]);
        if (len[g]) CHECK(ec_copy(p, plain[g], len[g]) == EC_OK, "ec_copy H2D");
        in[g] = len[g] ? p : NULL; /* (the plaintext of an empty message may be NULL) */
        out[g] = window(len[g] + TAG, out_shift[g], &b_sealed[g], &c_sealed[g]);
        cin[g] = out[g];
        back[g] = window(len[g], in_shift[g], &b_back[g], &c_back[g]);
        if (!len[g]) back[g] = NULL;
    }
    /* a NULL output: refused, nothing written */
    uint8_t *out_bad[NMSG] = {out[0], NULL, out[2]};
    rc = ec_gcm_seal_messages(ctx, NMSG, in, len, d_keys, d_nonces, out_bad, NULL);
    CHECK(rc == EC_ERR_INVALID_ARG, "a NULL output: rc %d", rc);
    rc = ec_gcm_seal_messages(ctx, NMSG, in, len, d_keys, d_nonces, out, NULL);
    CHECK(rc == EC_OK, "ec_gcm_seal_messages rc %d (%s)", rc, ec_strerror(rc));
    for (int g = 0; g < NMSG; g++) check_window("sealed message", g, b_sealed[g], c_sealed[g], out_shift[g], sealed[g], len[g] + TAG);

    int32_t status[NMSG] = {7, 7, 7};
    rc = ec_gcm_open_messages(ctx, NMSG, cin, len, d_keys, d_nonces, back, d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_messages rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status"); /* (waits for the default stream) */
    for (int g = 0; g < NMSG; g++) {
        CHECK(status[g] == 0, "message %d: status %d", g, (int)status[g]);
        check_window("opened message", g, b_back[g], c_back[g], in_shift[g], plain[g], len[g]);
    }
    /* a tag bit of message 1: status 1 and 32 zero bytes for it, the others as before */
    uint8_t flipped = sealed[1][len[1] + 5] ^ 0x08;
    CHECK(ec_copy(out[1] + len[1] + 5, &flipped, 1) == EC_OK, "ec_copy bit");
    rc = ec_gcm_open_messages(ctx, NMSG, cin, len, d_keys, d_nonces, back, d_status, NULL);
    CHECK(rc == EC_OK, "ec_gcm_open_messages rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof status) == EC_OK, "ec_copy status");
    CHECK(status[0] == 0 && status[1] == 1 && status[2] == 0, "status %d %d %d after a flipped tag bit", (int)status[0],
          (int)status[1], (int)status[2]);
    uint8_t zeros[32] = {0};
    check_window("opened message", 0, b_back[0], c_back[0], in_shift[0], plain[0], len[0]);
    check_window("tampered message", 1, b_back[1], c_back[1], in_shift[1], zeros, len[1]);

    unsigned long long seals = 9, opens = 9, passes = 9, per_pass = 0;
    CHECK(ec_gcm_messages_stats(ctx, &seals, &opens, &passes, &per_pass) == EC_OK, "ec_gcm_messages_stats");
    CHECK(seals == 1 && opens == 2 && passes == 3 && per_pass >= NMSG, "launches %llu + %llu, passes %llu of %llu", seals,
          opens, passes, per_pass);
    for (int g = 0; g < NMSG; g++) {
        ec_device_free(b_plain[g]);
        ec_device_free(b_sealed[g]);
        ec_device_free(b_back[g]);
        free(plain[g]);
        free(sealed[g]);
    }
    ec_device_free(d_kn);
    ec_device_free(d_status);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: %d messages of %zu, %zu and %zu bytes sealed and opened in one call each\n", NMSG, len[0], len[1], len[2]);
    return 0;
}
