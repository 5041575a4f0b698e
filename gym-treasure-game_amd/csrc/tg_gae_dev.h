// tg_gae_dev.h — k_gae: tg_gae.h's scan, one lane per env (tg_gae, tg_rollout_mlp_gae; DESIGN.md
// §13).  Compiled by tg_amd.hip only.
//
// A stream: per step a wave reads one coalesced row segment each of reward, done and value (and
// of vnext in the lanes whose step was truncated, when given) and writes adv, ret and vnext;
// value[s+1] stays in a register from the iteration before.  No LDS, no atomics.  The rows of
// GAE_UNROLL steps are loaded before the first of them is used, so a wave has that many rows in
// flight; what is computed is tg::gae_scan's, step by step in its order.
#pragma once
#include <hip/hip_runtime.h>

#include "tg_gae.h"

namespace {

constexpr int GAE_BLOCK = 256, GAE_UNROLL = 4;

template <bool STORE_VNEXT>
__global__ __launch_bounds__(GAE_BLOCK) void k_gae(int32_t steps, int64_t n, float gamma, float lambda,
                                                    const int32_t* __restrict__ reward,
                                                    const uint8_t* __restrict__ done,
                                                    const float* __restrict__ value, float* vnext,
                                                    const float* __restrict__ vboot, int vnext_given,
                                                    float* __restrict__ adv, float* __restrict__ ret) {
  const int64_t i = (int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float gl = gamma * lambda;
  float a = 0.0f, after = vboot[i];
  int32_t s = steps;
  for (; s >= GAE_UNROLL; s -= GAE_UNROLL) {  // steps s-1 .. s-GAE_UNROLL
    uint32_t d[GAE_UNROLL];
    int32_t r[GAE_UNROLL];
    float v[GAE_UNROLL], vt[GAE_UNROLL];
#pragma unroll
    for (int j = 0; j < GAE_UNROLL; ++j) {
      const int64_t k = (int64_t)(s - 1 - j) * n + i;
      d[j] = done[k];
      r[j] = reward[k];
      v[j] = value[k];
    }
#pragma unroll
    for (int j = 0; j < GAE_UNROLL; ++j) {
      const int64_t k = (int64_t)(s - 1 - j) * n + i;
      vt[j] = tg::gae_reads_vnext(d[j], vnext_given) ? vnext[k] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < GAE_UNROLL; ++j) {
      const int64_t k = (int64_t)(s - 1 - j) * n + i;
      const float nv = tg::gae_next_value(d[j], vnext_given, vt[j], after);
      ret[k] = tg::gae_step(gamma, gl, r[j], d[j], v[j], nv, a);
      adv[k] = a;
      if (STORE_VNEXT) vnext[k] = nv;
      after = v[j];
    }
  }
  for (--s; s >= 0; --s) {
    const int64_t k = (int64_t)s * n + i;
    const uint32_t d = done[k];
    const float v = value[k];
    const float vt = tg::gae_reads_vnext(d, vnext_given) ? vnext[k] : 0.0f;
    const float nv = tg::gae_next_value(d, vnext_given, vt, after);
    ret[k] = tg::gae_step(gamma, gl, reward[k], d, v, nv, a);
    adv[k] = a;
    if (STORE_VNEXT) vnext[k] = nv;
    after = v;
  }
}

}  // namespace
