// The geometry of the one-shot message cipher (uplink_amd/csrc/gcm_msg_geom.hpp)
// on its own: slot and round counts at every boundary length, where every padded
// slot of a message lands (front padding, data in order, the length block last on
// lane 63), the lanes that are live and the combine steps that follow from them,
// the pass split at kPassMessages and one either side, and that every message of
// a pass has exactly one (workgroup, wave) and no workgroup is empty.  Built by
// tests/test_messages_host.py with -fsanitize=address,undefined; prints "ok".
#include <cstdio>
#include <vector>

#include "gcm_msg_geom.hpp"

using namespace uplink_ec::gcmmsg;
using uplink_ec::sized::Pass;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "line %d: %s failed\n", __LINE__, #c);  \
            failures++;                                             \
        }                                                           \
    } while (0)

static void check_length(uint64_t len) {
    const uint32_t S = slots(len), R = rounds(len), pad = front_pad(len);
    CHECK(S == (len + 15) / 16 + 1);
    CHECK(R >= 1 && (uint64_t)R * kLanes >= S && (uint64_t)(R - 1) * kLanes < S);  // the fewest rounds that hold S slots
    CHECK(pad + S == R * kLanes && pad < kLanes);
    CHECK(tail_bytes(len) >= 1 && tail_bytes(len) <= 16);
    if (len) CHECK((uint64_t)(data_slots(len) - 1) * 16 + tail_bytes(len) == len);
    // every padded slot: padding first, then the data slots in order, the length block last; lanes take runs of R
    uint32_t next_data = 0, first_live = kLanes;
    if (R <= 4096) {
        for (uint32_t t = 0; t < R * kLanes; t++) {
            const Slot k = slot_kind(len, t);
            CHECK(lane_of(len, t) * R + round_of(len, t) == t && lane_of(len, t) < kLanes && round_of(len, t) < R);
            if (t < pad) {
                CHECK(k == Slot::kPad);
            } else if (t + 1 == R * kLanes) {
                CHECK(k == Slot::kLength && lane_of(len, t) == 63 && round_of(len, t) == R - 1);
            } else {
                CHECK(k == Slot::kData && t - pad == next_data);
                next_data++;
            }
            if (k != Slot::kPad && lane_of(len, t) < first_live) first_live = lane_of(len, t);
        }
        CHECK(next_data == data_slots(len));
        CHECK(kLanes - first_live == live_lanes(len));
    }
    // the steps: exactly those whose distance is below the live lanes
    const uint32_t live = live_lanes(len), steps = combine_steps(len);
    CHECK(live >= 1 && live <= kLanes && steps <= 6);
    CHECK((1u << steps) >= live);
    if (steps) CHECK((1u << (steps - 1)) < live);
}

int main() {
    const uint64_t lens[] = {0,    1,    15,   16,   17,   31,   32,   33,   47,   48,   49,   112,  113,  240,
                             241,  496,  497,  1007, 1008, 1009, 1023, 1024, 1025, 2032, 2033, 2053, 4095, 4096,
                             4097, 8191, 65535, 65536, kMaxLen - 1, kMaxLen};
    for (uint64_t len : lens) check_length(len);
    for (uint64_t len = 0; len <= 5000; len++) check_length(len);
    // the values the kernel's comments and the tests name
    CHECK(slots(0) == 1 && rounds(0) == 1 && front_pad(0) == 63 && live_lanes(0) == 1 && combine_steps(0) == 0);
    CHECK(slots(32) == 3 && live_lanes(32) == 3 && combine_steps(32) == 2);
    CHECK(slots(1008) == 64 && rounds(1008) == 1 && front_pad(1008) == 0 && combine_steps(1008) == 6);
    CHECK(slots(1009) == 65 && rounds(1009) == 2 && front_pad(1009) == 63 && live_lanes(1009) == 33);
    CHECK(rounds(2032) == 2 && front_pad(2032) == 0 && rounds(2033) == 3);
    CHECK(rounds(4096) == 5 && slots(4096) == 257 && front_pad(4096) == 63);
    CHECK(rounds(kMaxLen) == 16385);
    CHECK(kWgMessages == kWaves && kPassMessages % kWgMessages == 0);

    // passes: consecutive, full but the last, nothing lost
    const size_t P = kPassMessages;
    for (size_t n : {(size_t)0, (size_t)1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1}) {
        const std::vector<Pass> ps = split(n);
        CHECK(ps.size() == (n + P - 1) / P);
        size_t at = 0;
        for (size_t i = 0; i < ps.size(); i++) {
            CHECK(ps[i].i0 == at && ps[i].i1 > ps[i].i0 && ps[i].i1 - ps[i].i0 <= P);
            if (i + 1 < ps.size()) CHECK(ps[i].i1 - ps[i].i0 == P);
            at = ps[i].i1;
        }
        CHECK(at == n);
    }
    CHECK(split(10, 4).size() == 3 && split(10, 4)[2].i0 == 8 && split(10, 4)[2].i1 == 10);

    // workgroups: every message has one owner, no workgroup without a message
    for (size_t n : {(size_t)1, (size_t)3, (size_t)5, (size_t)kWaves - 1, (size_t)kWaves, (size_t)kWaves + 1, P - 1, P}) {
        const uint32_t wgs = pass_workgroups(n);
        std::vector<int> owners(n, 0);
        for (uint32_t wg = 0; wg < wgs; wg++) {
            int mine = 0;
            for (uint32_t w = 0; w < kWaves; w++) {
                const size_t q = message_of(wg, w, n);
                CHECK(q <= n);
                if (q < n) owners[q]++, mine++;
            }
            CHECK(mine >= 1);
        }
        for (size_t q = 0; q < n; q++) CHECK(owners[q] == 1);
    }
    CHECK(pass_workgroups(0) == 0);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
