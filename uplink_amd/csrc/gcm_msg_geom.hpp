// Geometry of an AES-256-GCM call over a list of one-shot messages
// (include/uplink_ec.h ec_gcm_seal_messages / ec_gcm_open_messages; kernel
// gcm_messages in aesgcm.hip): the GHASH slots of a length, the slots every lane
// of the message's wave takes, the zero slots in front, the combine steps a
// message needs, the messages of a workgroup and of a pass.  Plain C++, no HIP:
// tests/c/gcm_msg_geom_test.cpp compiles it on its own.
//
// A message of len bytes has slots(len) = ceil(len / 16) + 1 GHASH inputs: its
// ciphertext in 16-byte slots, the last one zero padded, then the length block.
// One wave takes the message.  Its 64 lanes each take rounds(len) consecutive
// slots of the 64 * rounds slots that start with front_pad(len) zero slots
// (leading zeros do not change a GHASH), so the length block is always the last
// slot of lane 63 and slot t of the message is padded slot front_pad + t.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sized_geom.hpp"

namespace uplink_ec {
namespace gcmmsg {

constexpr uint32_t kLanes = 64;           // lanes of the wave that takes a message
constexpr uint32_t kWaves = 8;            // waves of a workgroup: a message each (they share one fill of the AES tables)
constexpr uint32_t kWgMessages = kWaves;  // messages of a workgroup
constexpr size_t kPassMessages = 8192;    // messages of a pass: 24 bytes of staging and of descriptor each
constexpr uint64_t kMaxLen = 1ull << 24;  // bytes of one message
constexpr uint32_t kTagBytes = 16;

// 16-byte ciphertext slots of a message
constexpr uint32_t data_slots(uint64_t len) { return (uint32_t)((len + 15) / 16); }
// GHASH inputs: the ciphertext slots and the length block
constexpr uint32_t slots(uint64_t len) { return data_slots(len) + 1; }
// consecutive slots each lane takes (at least 1)
constexpr uint32_t rounds(uint64_t len) { return (slots(len) + kLanes - 1) / kLanes; }
// zero slots in front of the message's own
constexpr uint32_t front_pad(uint64_t len) { return rounds(len) * kLanes - slots(len); }
// lanes whose slots are not all front padding: the top `live` lanes of the wave
constexpr uint32_t live_lanes(uint64_t len) { return (slots(len) + rounds(len) - 1) / rounds(len); }
// Steps of the pairwise combination (distances 1, 2, 4, .. 32) the message needs:
// the step at distance d folds the d lanes below the top d into them, and is
// skipped when those hold only front padding (live_lanes <= d).
constexpr uint32_t combine_steps(uint64_t len) {
    uint32_t s = 0;
    while (s < 6 && live_lanes(len) > (1u << s)) s++;
    return s;
}
// bytes of the message's last ciphertext slot (16: a whole one; meaningless for len 0)
constexpr uint32_t tail_bytes(uint64_t len) { return len % 16 ? (uint32_t)(len % 16) : 16; }

// What padded slot t (0 .. 64 * rounds) of a message is.
enum class Slot { kPad, kData, kLength };
constexpr Slot slot_kind(uint64_t len, uint32_t t) {
    return t < front_pad(len) ? Slot::kPad : t + 1 == rounds(len) * kLanes ? Slot::kLength : Slot::kData;
}
// lane and round of padded slot t
constexpr uint32_t lane_of(uint64_t len, uint32_t t) { return t / rounds(len); }
constexpr uint32_t round_of(uint64_t len, uint32_t t) { return t % rounds(len); }

// Workgroups of a pass of n messages: message q of the pass belongs to wave
// q % kWaves of workgroup q / kWaves and to nobody else.
constexpr uint32_t pass_workgroups(size_t n) { return (uint32_t)((n + kWgMessages - 1) / kWgMessages); }
// the message of (workgroup, wave) in a pass of n, or n when the wave has none
constexpr size_t message_of(uint32_t wg, uint32_t wave, size_t n) {
    const size_t q = (size_t)wg * kWgMessages + wave;
    return q < n ? q : n;
}

// The passes of a list of n messages: consecutive messages, max_msgs each but the last.
inline std::vector<sized::Pass> split(size_t n, size_t max_msgs = kPassMessages) {
    std::vector<sized::Pass> out;
    for (size_t i0 = 0; i0 < n; i0 += max_msgs) out.push_back({i0, i0 + max_msgs < n ? i0 + max_msgs : n});
    return out;
}

}  // namespace gcmmsg
}  // namespace uplink_ec
