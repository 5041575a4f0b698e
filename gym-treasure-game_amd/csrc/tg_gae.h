// tg_gae.h — generalised advantage estimation over a rollout's step-major rows (tg_gae /
// tg_rollout_mlp_gae of include/tg_amd.h), one env at a time.  Shared by k_gae
// (tg_gae_dev.h) and by the host-only check build (tests/native_gae, plain g++): needs <math.h>
// and tg_hash.h (for TG_HD) only.
//
// Everything is f32 and every multiply-add is an explicit fmaf (the build has -ffp-contract=off),
// so an env's advantages depend on its own column alone: not on batch size, sharding, groups or
// tiling, and they are checkable bit for bit on the CPU.  For env i, s = K-1 .. 0, A_K = 0 and
// gl = gamma * lambda (one f32 product):
//
//   term  = done[s][i] & TERMINATED;  trunc = done[s][i] & TRUNCATED
//   nv    = term ? 0
//         : trunc && vnext_given ? vnext[s][i]            (V of the pre-reset state, given)
//         : s == K-1 ? vboot[i] : value[s+1][i]
//   delta = fmaf(gamma, nv, (float)reward[s][i]) - value[s][i]
//   carry = done[s][i] != 0 ? 0 : A_{s+1}
//   A_s   = fmaf(gl, carry, delta)
//   adv[s][i] = A_s;  ret[s][i] = A_s + value[s][i];  vnext[s][i] = nv
#pragma once
#include <math.h>
#include <stdint.h>

#include "tg_hash.h"  // TG_HD where the unit has not defined it (plain g++: inline)

namespace tg {

constexpr uint32_t GAE_TERMINATED = 1u, GAE_TRUNCATED = 2u;  // TG_DONE_*

TG_HD bool gae_coeff_ok(float c) { return c >= 0.0f && c <= 1.0f; }  // (false for a NaN)

// does step s's nv come from vnext[s][i]?  (the one load of vnext the scan makes)
TG_HD bool gae_reads_vnext(uint32_t d, int vnext_given) {
  return vnext_given && (d & GAE_TRUNCATED) && !(d & GAE_TERMINATED);
}

// nv of a step: vt is vnext[s][i] where gae_reads_vnext (else ignored), after is value[s+1][i]
// or vboot[i]
TG_HD float gae_next_value(uint32_t d, int vnext_given, float vt, float after) {
  if (d & GAE_TERMINATED) return 0.0f;
  return gae_reads_vnext(d, vnext_given) ? vt : after;
}

// A_s from A_{s+1} (a: in and out); returns ret
TG_HD float gae_step(float gamma, float gl, int32_t reward, uint32_t d, float v, float nv, float& a) {
  const float delta = fmaf(gamma, nv, (float)reward) - v;
  const float carry = d != 0u ? 0.0f : a;
  a = fmaf(gl, carry, delta);
  return a + v;
}

// env i's whole scan over [steps][n] rows (vnext may be null when !vnext_given: then not stored)
TG_HD void gae_scan(int32_t steps, int64_t n, int64_t i, float gamma, float lambda,
                    const int32_t* __restrict__ reward, const uint8_t* __restrict__ done,
                    const float* __restrict__ value, float* vnext, const float* __restrict__ vboot,
                    int vnext_given, float* __restrict__ adv, float* __restrict__ ret) {
  const float gl = gamma * lambda;
  float a = 0.0f, after = vboot[i];
  for (int32_t s = steps - 1; s >= 0; --s) {
    const int64_t k = (int64_t)s * n + i;
    const uint32_t d = done[k];
    const float v = value[k];
    const float vt = gae_reads_vnext(d, vnext_given) ? vnext[k] : 0.0f;
    const float nv = gae_next_value(d, vnext_given, vt, after);
    ret[k] = gae_step(gamma, gl, reward[k], d, v, nv, a);
    adv[k] = a;
    if (vnext) vnext[k] = nv;
    after = v;
  }
}

}  // namespace tg
