/* Plain-C client of ec_encode_segments_sized (include/uplink_ec.h): the cgo
 * view of one call for a batch of uploads of different sizes.  Three segments
 * of three sizes through ec_device_alloc / ec_copy: first given by their data
 * lengths (the call writes PadReader's padding, checked on each), then, already
 * padded, parity only.  Expected pieces are the CPU oracle's encode of the
 * padded segments.  Built and run by tests/test_encode_sized_c.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uplink_ec.h"

/* oracle (CPU restatement of storj.io/infectious) */
int or_new_fec(int k, int n, uint8_t *enc_matrix, uint8_t *vand_matrix);
int or_baseline_encode_segment(int k, int n, int ess, const uint8_t *enc, const uint8_t *seg, size_t stripes,
                               uint8_t *pieces, int threads);

static int failures = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            failures++;                               \
            fprintf(stderr, "FAIL: " __VA_ARGS__);    \
            fprintf(stderr, "\n");                    \
        }                                             \
    } while (0)

static uint32_t rng_state = 20261021u;
static uint32_t rnd(void) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

enum { K = 29, N = 80, ESS = 256, NSEG = 3, GUARD = 64, STRIPE = K * ESS };

int main(void) {
    /* under a block; a ragged 10.25 blocks, its data ending 4 bytes before a stripe's end; two blocks and a stripe */
    static const size_t stripes[NSEG] = {3, 41, 9};
    static const size_t data_len[NSEG] = {2 * STRIPE + 1, 41 * STRIPE - 4, 8 * STRIPE + 4000};
    ec_ctx *ctx = NULL;
    int rc = ec_create(K, N, ESS, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t *enc = malloc((size_t)N * K), *vand = malloc((size_t)N * K);
    or_new_fec(K, N, enc, vand);
    uint8_t *given[NSEG], *padded[NSEG], *want[NSEG], *d_segs[NSEG], *d_pieces[NSEG];
    size_t spad[NSEG], plen[NSEG];
    for (int g = 0; g < NSEG; g++) {
        spad[g] = stripes[g] * STRIPE;
        plen[g] = stripes[g] * ESS;
        /* as given: the data, then 0xEE where the padding goes; guards of 0xCD around it */
        given[g] = malloc(spad[g] + 2 * GUARD);
        memset(given[g], 0xCD, spad[g] + 2 * GUARD);
        memset(given[g] + GUARD, 0xEE, spad[g]);
        for (size_t i = 0; i < data_len[g]; i++) given[g][GUARD + i] = (uint8_t)rnd();
        /* PadReader: p bytes of value p, the last 4 p big-endian */
        const size_t p = spad[g] - data_len[g];
        CHECK(p >= 4 && p <= STRIPE + 3, "segment %d: %zu bytes of padding", g, p);
        padded[g] = malloc(spad[g] + 2 * GUARD);
        memcpy(padded[g], given[g], spad[g] + 2 * GUARD);
        memset(padded[g] + GUARD + data_len[g], (int)(p & 0xFF), p);
        for (int b = 0; b < 4; b++) padded[g][GUARD + spad[g] - 1 - b] = (uint8_t)(p >> (8 * b));
        want[g] = malloc((size_t)N * plen[g] + 2 * GUARD);
        memset(want[g], 0xCD, (size_t)N * plen[g] + 2 * GUARD);
        or_baseline_encode_segment(K, N, ESS, enc, padded[g] + GUARD, stripes[g], want[g] + GUARD, 1);
        d_segs[g] = ec_device_alloc(spad[g] + 2 * GUARD);
        d_pieces[g] = ec_device_alloc((size_t)N * plen[g] + 2 * GUARD);
        CHECK(d_segs[g] != NULL && d_pieces[g] != NULL, "ec_device_alloc");
        if (!d_segs[g] || !d_pieces[g]) return 1;
        CHECK(ec_copy(d_segs[g], given[g], spad[g] + 2 * GUARD) == EC_OK, "ec_copy H2D");
    }
    uint8_t *blank = malloc((size_t)N * plen[1] + 2 * GUARD), *back = malloc((size_t)N * plen[1] + 2 * GUARD);
    memset(blank, 0xCD, (size_t)N * plen[1] + 2 * GUARD);
    uint8_t *segs[NSEG], *outs[NSEG];
    for (int g = 0; g < NSEG; g++) {
        CHECK(ec_copy(d_pieces[g], blank, (size_t)N * plen[g] + 2 * GUARD) == EC_OK, "fill pieces");
        segs[g] = d_segs[g] + GUARD;
        outs[g] = d_pieces[g] + GUARD;
    }
    /* a data length that does not pad to its stripe count: refused, nothing written */
    size_t wrong[NSEG] = {data_len[0], data_len[1] + 1, data_len[2]};
    rc = ec_encode_segments_sized(ctx, NSEG, segs, stripes, wrong, outs, 0, NULL);
    CHECK(rc == EC_ERR_INVALID_ARG, "a wrong data_len: rc %d", rc);
    for (int g = 0; g < NSEG; g++) {
        CHECK(ec_copy(back, d_segs[g], spad[g] + 2 * GUARD) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(back, given[g], spad[g] + 2 * GUARD) == 0, "segment %d written by a refused call", g);
        CHECK(ec_copy(back, d_pieces[g], (size_t)N * plen[g] + 2 * GUARD) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(back, blank, (size_t)N * plen[g] + 2 * GUARD) == 0, "pieces %d written by a refused call", g);
    }
    rc = ec_encode_segments_sized(ctx, NSEG, segs, stripes, data_len, outs, 0, NULL);
    CHECK(rc == EC_OK, "ec_encode_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    for (int g = 0; g < NSEG; g++) {
        CHECK(ec_copy(back, d_segs[g], spad[g] + 2 * GUARD) == EC_OK, "ec_copy D2H"); /* (waits for the default stream) */
        CHECK(memcmp(back, padded[g], spad[g] + 2 * GUARD) == 0, "segment %d: padding differs", g);
        CHECK(ec_copy(back, d_pieces[g], (size_t)N * plen[g] + 2 * GUARD) == EC_OK, "ec_copy D2H");
        for (size_t i = 0; i < (size_t)N * plen[g] + 2 * GUARD; i++)
            if (back[i] != want[g][i]) {
                CHECK(0, "segment %d piece byte %zu: %#x != %#x", g, i - GUARD, back[i], want[g][i]);
                break;
            }
    }
    /* already padded, parity only, the segments in another order: [n-k][piece_len] each */
    uint8_t *segs2[NSEG] = {segs[2], segs[0], segs[1]}, *outs2[NSEG] = {outs[2], outs[0], outs[1]};
    const size_t stripes2[NSEG] = {stripes[2], stripes[0], stripes[1]};
    for (int g = 0; g < NSEG; g++)
        CHECK(ec_copy(d_pieces[g], blank, (size_t)N * plen[g] + 2 * GUARD) == EC_OK, "refill pieces");
    rc = ec_encode_segments_sized(ctx, NSEG, segs2, stripes2, NULL, outs2, EC_FLAG_PARITY_ONLY, NULL);
    CHECK(rc == EC_OK, "parity only rc %d (%s)", rc, ec_strerror(rc));
    for (int g = 0; g < NSEG; g++) {
        const size_t par = (size_t)(N - K) * plen[g];
        CHECK(ec_copy(back, d_pieces[g], (size_t)N * plen[g] + 2 * GUARD) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(back + GUARD, want[g] + GUARD + (size_t)K * plen[g], par) == 0, "segment %d: parity differs", g);
        CHECK(memcmp(back, blank, GUARD) == 0 &&
                  memcmp(back + GUARD + par, blank, (size_t)N * plen[g] + GUARD - par) == 0,
              "segment %d: parity only wrote outside its %d pieces", g, N - K);
        CHECK(ec_copy(back, d_segs[g], spad[g] + 2 * GUARD) == EC_OK, "ec_copy D2H");
        CHECK(memcmp(back, padded[g], spad[g] + 2 * GUARD) == 0, "segment %d: an input was written", g);
    }
    for (int g = 0; g < NSEG; g++) {
        ec_device_free(d_segs[g]);
        ec_device_free(d_pieces[g]);
    }
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: one sized encode of %d segments of %zu, %zu and %zu stripes from their data lengths, one parity only\n",
           NSEG, stripes[0], stripes[1], stripes[2]);
    return 0;
}
