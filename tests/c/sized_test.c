/* Plain-C client of ec_rebuild_segments_sized (include/uplink_ec.h): the cgo
 * view of one call for a batch of downloads of different sizes.  Three
 * segments of three sizes, each from a share set of its own, through
 * ec_device_alloc / ec_copy; every expected segment is this program's own
 * input, its pieces the CPU oracle's.  Built and run by tests/test_sized_c.py. */
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

enum { K = 29, N = 80, ESS = 256, NSEG = 3, GUARD = 64 };

int main(void) {
    static const size_t stripes[NSEG] = {3, 41, 9}; /* less than a tile, a ragged 5.1 tiles, one tile and a stripe */
    ec_ctx *ctx = NULL;
    int rc = ec_create(K, N, ESS, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t *enc = malloc((size_t)N * K), *vand = malloc((size_t)N * K);
    or_new_fec(K, N, enc, vand);
    uint8_t *segs[NSEG], *pieces[NSEG], *d_pieces[NSEG];
    size_t spad[NSEG], plen[NSEG], out_off[NSEG], total = GUARD;
    for (int g = 0; g < NSEG; g++) {
        spad[g] = stripes[g] * K * ESS;
        plen[g] = stripes[g] * ESS;
        segs[g] = malloc(spad[g]);
        for (size_t i = 0; i < spad[g]; i++) segs[g][i] = (uint8_t)rnd();
        pieces[g] = malloc((size_t)N * plen[g]);
        or_baseline_encode_segment(K, N, ESS, enc, segs[g], stripes[g], pieces[g], 1);
        d_pieces[g] = ec_device_alloc((size_t)N * plen[g]);
        CHECK(d_pieces[g] != NULL, "ec_device_alloc");
        if (!d_pieces[g]) return 1;
        CHECK(ec_copy(d_pieces[g], pieces[g], (size_t)N * plen[g]) == EC_OK, "ec_copy H2D");
        out_off[g] = total;
        total += spad[g] + GUARD;
    }
    /* the outputs in one 0xCD-filled buffer with guards before, between and after */
    uint8_t *want = malloc(total), *blank = malloc(total), *back = malloc(total), *d_out = ec_device_alloc(total);
    CHECK(d_out != NULL, "ec_device_alloc");
    if (!d_out) return 1;
    memset(want, 0xCD, total);
    memset(blank, 0xCD, total);
    CHECK(ec_copy(d_out, blank, total) == EC_OK, "fill outputs");
    /* segment 0: the last k shares (all parity); 1: a shuffled random k-subset; 2: k + 3 shares, unsorted */
    int ns[NSEG] = {K, K, K + 3}, nums[3 * K + 3], w = 0;
    const uint8_t *ptrs[3 * K + 3];
    uint8_t *outs[NSEG];
    for (int g = 0; g < NSEG; g++) {
        int perm[N];
        for (int i = 0; i < N; i++) perm[i] = i;
        for (int i = N - 1; i > 0; i--) {
            int j = (int)(rnd() % (uint32_t)(i + 1)), t = perm[i];
            perm[i] = perm[j];
            perm[j] = t;
        }
        for (int i = 0; i < ns[g]; i++, w++) {
            nums[w] = g == 0 ? N - 1 - i : perm[i];
            ptrs[w] = d_pieces[g] + (size_t)nums[w] * plen[g];
        }
        outs[g] = d_out + out_off[g];
        memcpy(want + out_off[g], segs[g], spad[g]);
    }
    rc = ec_rebuild_segments_sized(ctx, NSEG, ns, nums, ptrs, stripes, outs, NULL);
    CHECK(rc == EC_OK, "ec_rebuild_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(back, d_out, total) == EC_OK, "ec_copy D2H"); /* (waits for the default stream) */
    for (size_t i = 0; i < total; i++)
        if (back[i] != want[i]) {
            CHECK(0, "output byte %zu: %#x != %#x", i, back[i], want[i]);
            break;
        }
    /* a Decode of the same batch: every segment's own outcome */
    int seg_rc[NSEG] = {7, 7, 7};
    CHECK(ec_copy(d_out, blank, total) == EC_OK, "refill");
    rc = ec_decode_segments_sized(ctx, NSEG, ns, nums, (uint8_t *const *)ptrs, stripes, outs, seg_rc, NULL);
    CHECK(rc == EC_OK && seg_rc[0] == EC_OK && seg_rc[1] == EC_OK && seg_rc[2] == EC_OK,
          "ec_decode_segments_sized rc %d (%d %d %d)", rc, seg_rc[0], seg_rc[1], seg_rc[2]);
    CHECK(ec_copy(back, d_out, total) == EC_OK, "ec_copy D2H");
    CHECK(memcmp(back, want, total) == 0, "decode output differs");
    for (int g = 0; g < NSEG; g++) ec_device_free(d_pieces[g]);
    ec_device_free(d_out);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: one sized Rebuild and one sized Decode of %d segments of %zu, %zu and %zu stripes\n", NSEG, stripes[0],
           stripes[1], stripes[2]);
    return 0;
}
