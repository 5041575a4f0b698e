// tg_srv_word.h — the N = 1 server's command word: its encoder (the host's, tg_amd.hip) and its
// decoders (k_serve1's, tg_py1.h) side by side.  Plain C++ with no HIP types, so the host checks
// (tests/native) compile the very functions the library and the kernel use.  The functions are
// constexpr: usable from host and device code alike.
#pragma once
#include <stdint.h>

namespace tg {

enum : uint32_t { SRV_STEP = 1, SRV_STEP_PY = 2, SRV_RESET_PY = 3, SRV_QUIT = 4, SRV_MASK = 5,
                  SRV_RESET = 6 };

// The action's 5-bit field holds action + 16 for the valid range [-9, 8] (codes 7..24).  Every
// other action, INT32_MIN and INT32_MAX included, is sent as code 0, which decodes to
// SRV_ACT_INVALID = -16: out of range again, so the server's step raises TG_ERR_ACTION and
// returns valid = 0 exactly as k_step / k_py1 do for the caller's own value.  (The range test
// comes before the addition: nothing overflows.)
constexpr int32_t SRV_ACT_MIN = -9, SRV_ACT_MAX = 8, SRV_ACT_INVALID = -16;
constexpr uint32_t srv_act_encode(int32_t action) {
  return action < SRV_ACT_MIN || action > SRV_ACT_MAX ? 0u : (uint32_t)(action + 16);
}
constexpr int32_t srv_act_decode(uint32_t code) { return (int32_t)(code & 31u) - 16; }

// the command word: kind | action code << 4 | warm << 9 | has_gauss << 10 | q0 << 11
constexpr uint32_t srv_word(uint32_t kind, int32_t action, bool warm, bool has_gauss, uint32_t q0) {
  return kind | srv_act_encode(action) << 4 | (warm ? 1u : 0u) << 9 |
         (has_gauss ? 1u : 0u) << 10 | (q0 & 1023u) << 11;
}
constexpr uint32_t srv_kind(uint32_t word) { return word & 15u; }
constexpr int32_t srv_action(uint32_t word) { return srv_act_decode(word >> 4); }
constexpr bool srv_warm(uint32_t word) { return (word >> 9) & 1u; }
constexpr bool srv_has_gauss(uint32_t word) { return (word >> 10) & 1u; }
constexpr uint32_t srv_q0(uint32_t word) { return word >> 11; }

static_assert(srv_action(srv_word(SRV_STEP, SRV_ACT_MIN, true, true, 624u)) == SRV_ACT_MIN &&
                  srv_action(srv_word(SRV_STEP, SRV_ACT_MAX, true, true, 624u)) == SRV_ACT_MAX,
              "the valid actions survive the word");
static_assert(srv_act_decode(srv_act_encode(SRV_ACT_MAX + 1)) == SRV_ACT_INVALID &&
                  srv_act_decode(srv_act_encode(SRV_ACT_MIN - 1)) == SRV_ACT_INVALID,
              "an action out of range stays out of range");
static_assert(SRV_ACT_INVALID < SRV_ACT_MIN, "the invalid code's action is out of range");

}  // namespace tg
