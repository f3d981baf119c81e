/* Plain-C client of ec_repair_segments_sized (include/uplink_ec.h): the cgo view
 * of one call for a repair queue of segments of different sizes.  Three
 * segments of three sizes, each with a share set and a target set of its own,
 * through ec_device_alloc / ec_copy, with the share check on; every expected
 * piece is the CPU oracle's.  Built and run by tests/test_repair_sized_c.py. */
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

static uint32_t rng_state = 20261020u;
static uint32_t rnd(void) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

enum { K = 29, N = 80, ESS = 256, NSEG = 3, GUARD = 64, MAXT = N - K };

int main(void) {
    static const size_t stripes[NSEG] = {3, 41, 9}; /* less than a tile, a ragged 5.1 tiles, one tile and a stripe */
    static const int ns[NSEG] = {K, K + 3, K + 20};  /* shares given: the basis, and a surplus the check compares */
    static const int nt[NSEG] = {51, 5, 20};         /* 8, 2 and 8 waves (20 + 20 syndrome rows) */
    ec_ctx *ctx = NULL;
    int rc = ec_create(K, N, ESS, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t *enc = malloc((size_t)N * K), *vand = malloc((size_t)N * K);
    or_new_fec(K, N, enc, vand);
    uint8_t *pieces[NSEG], *d_pieces[NSEG];
    size_t plen[NSEG];
    for (int g = 0; g < NSEG; g++) {
        const size_t spad = stripes[g] * K * ESS;
        plen[g] = stripes[g] * ESS;
        uint8_t *seg = malloc(spad);
        for (size_t i = 0; i < spad; i++) seg[i] = (uint8_t)rnd();
        pieces[g] = malloc((size_t)N * plen[g]);
        or_baseline_encode_segment(K, N, ESS, enc, seg, stripes[g], pieces[g], 1);
        free(seg);
        d_pieces[g] = ec_device_alloc((size_t)N * plen[g]);
        CHECK(d_pieces[g] != NULL, "ec_device_alloc");
        if (!d_pieces[g]) return 1;
        CHECK(ec_copy(d_pieces[g], pieces[g], (size_t)N * plen[g]) == EC_OK, "ec_copy H2D");
    }
    /* per segment a shuffled share set and targets among the other pieces; the outputs in one
     * 0xCD-filled buffer with guards before, between and after */
    int nums[NSEG * N], targets[NSEG * MAXT], w = 0, t = 0;
    const uint8_t *ptrs[NSEG * N];
    size_t out_off[NSEG * MAXT], total = GUARD;
    for (int g = 0; g < NSEG; g++) {
        int perm[N];
        for (int i = 0; i < N; i++) perm[i] = i;
        for (int i = N - 1; i > 0; i--) {
            int j = (int)(rnd() % (uint32_t)(i + 1)), x = perm[i];
            perm[i] = perm[j];
            perm[j] = x;
        }
        for (int i = 0; i < ns[g]; i++, w++) {
            nums[w] = perm[i];
            ptrs[w] = d_pieces[g] + (size_t)nums[w] * plen[g];
        }
        for (int i = 0; i < nt[g]; i++, t++) {
            targets[t] = perm[ns[g] + i];
            out_off[t] = total;
            total += plen[g] + GUARD;
        }
    }
    uint8_t *want = malloc(total), *back = malloc(total), *d_out = ec_device_alloc(total);
    int32_t *d_status = ec_device_alloc(NSEG * sizeof(int32_t));
    CHECK(d_out != NULL && d_status != NULL, "ec_device_alloc");
    if (!d_out || !d_status) return 1;
    memset(want, 0xCD, total);
    CHECK(ec_copy(d_out, want, total) == EC_OK, "fill outputs");
    int32_t status[NSEG] = {7, 7, 7};
    CHECK(ec_copy(d_status, status, sizeof(status)) == EC_OK, "fill status");
    uint8_t *outs[NSEG * MAXT];
    t = 0;
    for (int g = 0; g < NSEG; g++)
        for (int i = 0; i < nt[g]; i++, t++) {
            outs[t] = d_out + out_off[t];
            memcpy(want + out_off[t], pieces[g] + (size_t)targets[t] * plen[g], plen[g]);
        }
    rc = ec_repair_segments_sized(ctx, NSEG, ns, nums, ptrs, nt, targets, outs, stripes, EC_FLAG_CHECK_SHARES, d_status,
                                  NULL);
    CHECK(rc == EC_OK, "ec_repair_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(back, d_out, total) == EC_OK, "ec_copy D2H"); /* (waits for the default stream) */
    for (size_t i = 0; i < total; i++)
        if (back[i] != want[i]) {
            CHECK(0, "output byte %zu: %#x != %#x", i, back[i], want[i]);
            break;
        }
    CHECK(ec_copy(status, d_status, sizeof(status)) == EC_OK, "ec_copy status");
    CHECK(status[0] == 0 && status[1] == 0 && status[2] == 0, "status %d %d %d", status[0], status[1], status[2]);
    /* one byte of segment 1's last share flipped in its last column: flagged, the others not */
    uint8_t bad = (uint8_t)(pieces[1][(size_t)nums[ns[0] + ns[1] - 1] * plen[1] + plen[1] - 1] ^ 0x40);
    CHECK(ec_copy((uint8_t *)ptrs[ns[0] + ns[1] - 1] + plen[1] - 1, &bad, 1) == EC_OK, "damage a share");
    rc = ec_repair_segments_sized(ctx, NSEG, ns, nums, ptrs, nt, targets, outs, stripes, EC_FLAG_CHECK_SHARES, d_status,
                                  NULL);
    CHECK(rc == EC_OK, "second ec_repair_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(status, d_status, sizeof(status)) == EC_OK, "ec_copy status");
    CHECK(status[0] == 0 && status[1] == 1 && status[2] == 0, "status after damage %d %d %d", status[0], status[1],
          status[2]);
    for (int g = 0; g < NSEG; g++) ec_device_free(d_pieces[g]);
    ec_device_free(d_out);
    ec_device_free(d_status);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: one sized repair of %d segments of %zu, %zu and %zu stripes, share check on\n", NSEG, stripes[0],
           stripes[1], stripes[2]);
    return 0;
}
