// tg_hostcheck_gae.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the advantage scan (gym-treasure-game_amd/csrc/tg_gae.h) over arrays: the
// function k_gae restates per lane, so the tests can hold the device's adv, ret and vnext to it
// bit for bit and check it against an independent float64 scan.  The product library never
// contains or calls this.  Built by tests/native_gae/Makefile with g++ and -ffp-contract=off.
#include <cstdint>

#include "../../gym-treasure-game_amd/csrc/tg_gae.h"

extern "C" {

// tg_gae's arguments over host rows [steps][n]; vnext may be null when !vnext_given.  Returns -1
// for what tg_gae rejects.
int hg_gae(int32_t steps, int64_t n, float gamma, float lambda, const int32_t* reward,
           const uint8_t* done, const float* value, float* vnext, const float* vboot,
           int32_t vnext_given, float* adv, float* ret) {
  if (!tg::gae_coeff_ok(gamma) || !tg::gae_coeff_ok(lambda) || steps < 0 || n < 0) return -1;
  if (!reward || !done || !value || !vboot || !adv || !ret || (vnext_given && !vnext)) return -1;
  for (int64_t i = 0; i < n; ++i)
    tg::gae_scan(steps, n, i, gamma, lambda, reward, done, value, vnext, vboot, vnext_given ? 1 : 0, adv,
                 ret);
  return 0;
}

}  // extern "C"
