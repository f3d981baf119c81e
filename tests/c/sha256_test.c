/* Plain-C client of ec_sha256_segments_sized and ec_sha256_pieces_list
 * (include/uplink_ec.h): the cgo view of the SHA-256 piece hashes of a batch of
 * uploads of different sizes.  Three segments of three sizes through
 * ec_device_alloc / ec_copy: one ec_encode_segments_sized (parity only), one
 * ec_sha256_segments_sized over the same arguments, and one
 * ec_sha256_pieces_list over three windows of the first segment, one of them
 * empty.  The segments are a fixed generator's bytes; the expected digests come
 * from the test that runs this program (hashlib's, over the oracle's pieces), as
 * hexadecimal arguments: argv[1] the [NSEG][N][32] segment digests, argv[2] the
 * three list digests.  Built and run by tests/test_sha256_c.py. */
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

enum { K = 29, N = 80, ESS = 256, NSEG = 3, NLIST = 3, GUARD = 64, STRIPE = K * ESS };

/* byte i of segment g (the test generates the same) */
static uint8_t seg_byte(int g, size_t i) { return (uint8_t)((i * 2654435761u + (size_t)g * 40503u) >> 11); }

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
    static const size_t stripes[NSEG] = {3, 1025, 41}; /* pieces of 768, 262,400 and 10,496 bytes */
    /* windows of segment 0: an aligned one, one at an odd address, an empty one */
    static const size_t list_off[NLIST] = {0, 4097, 0}, list_len[NLIST] = {4096, 3000, 0};
    static uint8_t want_seg[NSEG * N * 32], want_list[NLIST * 32];
    if (argc != 3 || unhex(argv[1], want_seg, sizeof want_seg) || unhex(argv[2], want_list, sizeof want_list)) {
        fprintf(stderr, "usage: sha256_test <segment digests, hex> <list digests, hex>\n");
        return 2;
    }
    ec_ctx *ctx = NULL;
    int rc = ec_create(K, N, ESS, &ctx);
    CHECK(rc == EC_OK, "ec_create rc %d (%s)", rc, ec_strerror(rc));
    if (rc) return 1;
    uint8_t *d_segs[NSEG], *d_par[NSEG];
    const uint8_t *segs[NSEG], *pars[NSEG];
    uint8_t *enc_in[NSEG], *enc_out[NSEG];
    for (int g = 0; g < NSEG; g++) {
        const size_t bytes = stripes[g] * STRIPE, pbytes = (size_t)(N - K) * stripes[g] * ESS;
        uint8_t *h = malloc(bytes);
        for (size_t i = 0; i < bytes; i++) h[i] = seg_byte(g, i);
        d_segs[g] = ec_device_alloc(bytes);
        d_par[g] = ec_device_alloc(pbytes);
        CHECK(d_segs[g] != NULL && d_par[g] != NULL, "ec_device_alloc");
        if (!d_segs[g] || !d_par[g]) return 1;
        CHECK(ec_copy(d_segs[g], h, bytes) == EC_OK, "ec_copy H2D");
        free(h);
        segs[g] = enc_in[g] = d_segs[g];
        pars[g] = enc_out[g] = d_par[g];
    }
    /* the hash buffer between two guards of 0xCD */
    const size_t hbytes = (size_t)NSEG * N * 32 + 2 * GUARD;
    uint8_t *blank = malloc(hbytes), *back = malloc(hbytes);
    memset(blank, 0xCD, hbytes);
    uint8_t *d_hash = ec_device_alloc(hbytes);
    CHECK(d_hash != NULL, "ec_device_alloc");
    if (!d_hash) return 1;
    CHECK(ec_copy(d_hash, blank, hbytes) == EC_OK, "fill hashes");
    rc = ec_encode_segments_sized(ctx, NSEG, enc_in, stripes, NULL, enc_out, EC_FLAG_PARITY_ONLY, NULL);
    CHECK(rc == EC_OK, "ec_encode_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    /* a segment without its parity pieces: refused, nothing written */
    const uint8_t *pars_bad[NSEG] = {pars[0], NULL, pars[2]};
    rc = ec_sha256_segments_sized(ctx, NSEG, segs, stripes, pars_bad, EC_FLAG_PARITY_ONLY, d_hash + GUARD, NULL);
    CHECK(rc == EC_ERR_INVALID_ARG, "a NULL pieces[1]: rc %d", rc);
    CHECK(ec_copy(back, d_hash, hbytes) == EC_OK, "ec_copy D2H");
    CHECK(memcmp(back, blank, hbytes) == 0, "hashes written by a refused call");
    rc = ec_sha256_segments_sized(ctx, NSEG, segs, stripes, pars, EC_FLAG_PARITY_ONLY, d_hash + GUARD, NULL);
    CHECK(rc == EC_OK, "ec_sha256_segments_sized rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(back, d_hash, hbytes) == EC_OK, "ec_copy D2H"); /* (waits for the default stream) */
    CHECK(memcmp(back, blank, GUARD) == 0 && memcmp(back + hbytes - GUARD, blank, GUARD) == 0, "a guard was written");
    for (int g = 0; g < NSEG; g++)
        for (int j = 0; j < N; j++)
            CHECK(memcmp(back + GUARD + ((size_t)g * N + j) * 32, want_seg + ((size_t)g * N + j) * 32, 32) == 0,
                  "segment %d piece %d: digest differs", g, j);
    /* the list form: three windows of segment 0 */
    const uint8_t *lp[NLIST];
    for (int i = 0; i < NLIST; i++) lp[i] = list_len[i] ? d_segs[0] + list_off[i] : NULL;
    CHECK(ec_copy(d_hash, blank, hbytes) == EC_OK, "refill hashes");
    rc = ec_sha256_pieces_list(ctx, NLIST, lp, list_len, d_hash + GUARD, NULL);
    CHECK(rc == EC_OK, "ec_sha256_pieces_list rc %d (%s)", rc, ec_strerror(rc));
    CHECK(ec_copy(back, d_hash, hbytes) == EC_OK, "ec_copy D2H");
    CHECK(memcmp(back + GUARD, want_list, NLIST * 32) == 0, "list digests differ");
    CHECK(memcmp(back, blank, GUARD) == 0 && memcmp(back + GUARD + NLIST * 32, blank, hbytes - GUARD - NLIST * 32) == 0,
          "the list call wrote outside its %d rows", NLIST);
    unsigned long long fast = 0, bytewise = 0, launches = 0;
    CHECK(ec_sha256_list_stats(ctx, &fast, &bytewise, &launches) == EC_OK, "ec_sha256_list_stats");
    /* 240 pieces, all on the 16-byte loads, and the aligned and the empty window; the odd window bytewise */
    CHECK(fast == NSEG * N + 2 && bytewise == 1 && launches == 2, "stats %llu %llu %llu", fast, bytewise, launches);
    CHECK(EC_HASH_SHA256 == 0 && EC_HASH_BLAKE3 == 1, "pb.PieceHashAlgorithm values");
    for (int g = 0; g < NSEG; g++) {
        ec_device_free(d_segs[g]);
        ec_device_free(d_par[g]);
    }
    ec_device_free(d_hash);
    ec_destroy(ctx);
    if (failures) return 1;
    printf("ok: the %d SHA-256 piece hashes of %d segments of %zu, %zu and %zu stripes in one call, and a list of %d pieces\n",
           NSEG * N, NSEG, stripes[0], stripes[1], stripes[2], NLIST);
    return 0;
}
