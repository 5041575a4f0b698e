// tg_policy_mlp.h — the learned actor's arithmetic (tg_policy_mlp / tg_rollout_mlp of
// include/tg_amd.h), one env at a time.  Shared by k_policy_mlp (tg_kernels.h) and by
// the host-only check build (tests/native_policy, plain g++): needs <math.h> and tg_hash.h only.
//
// Everything is f32 and every multiply-add is an explicit fmaf in a fixed order (the build has
// -ffp-contract=off), so logits and value do not depend on batch size, sharding or tiling and are
// checkable bit for bit on the CPU.  chain(c; w, x): for k ascending, c = fmaf(w[k], x[k], c).
//
//   x[j]     = fmaf((float)o[j], obs_scale[j], obs_shift[j])       o: tg_observe's f64 row
//   a1[i]    = act(chain(b1[i]; W1[i], x))
//   a2[i]    = act(chain(b2[i]; W2[i], a1))
//   logit[k] = chain(bp[k]; Wp[k], a2)
//   value    = chain(bv; Wv, a2)
//
// The heads' chains run over a2 in ascending i, so they are advanced as each a2[i] is produced
// and a2 is never stored: the evaluation keeps x, a1 and ten accumulators live.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tg_hash.h"  // sm64, and TG_HD where the unit has not defined it (plain g++: inline)

namespace tg {

constexpr int MLP_IN = 9, MLP_OUT = 9;
constexpr int MLP_MAX_HIDDEN = 128;
constexpr int MLP_ACT_RELU = 0, MLP_ACT_TANH = 1;  // TG_ACT_*
constexpr int MLP_SAMPLE = 0, MLP_GREEDY = 1;      // TG_MLP_*

TG_HD bool mlp_hidden_ok(int h) { return h == 16 || h == 32 || h == 64 || h == 128; }
// packed parameters: obs_scale[9], obs_shift[9], W1[H][9], b1[H], W2[H][H], b2[H], Wp[9][H],
// bp[9], Wv[H], bv[1]
TG_HD int mlp_param_count(int h) { return h * h + 21 * h + 28; }
template <int H>
struct MlpLayout {
  static constexpr int SCALE = 0, SHIFT = 9, W1 = 18, B1 = W1 + 9 * H, W2 = B1 + H,
                       B2 = W2 + H * H, WP = B2 + H, BP = WP + 9 * H, WV = BP + 9, BV = WV + H,
                       COUNT = BV + 1;
  static_assert(COUNT == H * H + 21 * H + 28, "packed parameter count");
};

// the host check only: tanh by the double library, rounded to f32 (the sensitivity of the outputs
// to activations that differ in the last place)
constexpr int MLP_ACT_TANH_F64 = 2;

template <int ACT>
TG_HD float mlp_act(float z) {
  if (ACT == MLP_ACT_TANH) return tanhf(z);
  if (ACT == MLP_ACT_TANH_F64) return (float)tanh((double)z);
  return z > 0.0f ? z : 0.0f;
}

// logits and value of one env from its observation row.  p: the packed parameters (on the
// device a wave-uniform address: the weights are scalar loads).
template <int H, int ACT>
TG_HD void mlp_forward(const float* __restrict__ p, const double o[9], float logit[9],
                       float& value) {
  using Y = MlpLayout<H>;
  float x[MLP_IN];
#pragma unroll
  for (int j = 0; j < MLP_IN; ++j) x[j] = fmaf((float)o[j], p[Y::SCALE + j], p[Y::SHIFT + j]);
  float a1[H];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float c = p[Y::B1 + i];
#pragma unroll
    for (int k = 0; k < MLP_IN; ++k) c = fmaf(p[Y::W1 + i * MLP_IN + k], x[k], c);
    a1[i] = mlp_act<ACT>(c);
  }
  float lg[MLP_OUT];
#pragma unroll
  for (int k = 0; k < MLP_OUT; ++k) lg[k] = p[Y::BP + k];
  float v = p[Y::BV];
#pragma unroll 2
  for (int i = 0; i < H; ++i) {
    const float* __restrict__ w = p + Y::W2 + i * H;
    float c = p[Y::B2 + i];
#pragma unroll
    for (int k = 0; k < H; ++k) c = fmaf(w[k], a1[k], c);
    const float a2 = mlp_act<ACT>(c);
#pragma unroll
    for (int k = 0; k < MLP_OUT; ++k) lg[k] = fmaf(p[Y::WP + k * H + i], a2, lg[k]);
    v = fmaf(p[Y::WV + i], a2, v);
  }
#pragma unroll
  for (int k = 0; k < MLP_OUT; ++k) logit[k] = lg[k];
  value = v;
}

// the allowed set A as bits: the env's available_mask when `masked` and it is non-zero, else
// all nine actions (TG_POLICY_MASKED's fallback)
TG_HD uint32_t mlp_allowed(int masked, uint32_t avail) {
  const uint32_t a = avail & 0x1FFu;
  return (masked && a) ? a : 0x1FFu;
}

// u in [0, 1) of (action seed, GLOBAL env index, step): the top 24 bits of policy_action's hash
TG_HD float mlp_uniform(uint64_t a0, int64_t g, int64_t t) {
  const uint64_t h = sm64(sm64(a0 ^ sm64((uint64_t)g)) ^ (uint64_t)t);
  return (float)(h >> 40) * 0x1p-24f;
}

// The action over A (allowed: non-zero, bits 0..8) and its log-probability.
//   m = max logit over A; e[k] = expf(logit[k] - m); Z = the f32 sum of e over A, ascending;
//   sample: the first k in A whose running sum exceeds u * Z, else the last k in A;
//   greedy: the lowest k in A with logit[k] == m;  logp = (logit[a] - m) - logf(Z).
// Every index comes from A's bits, whatever the floats hold.
TG_HD int mlp_select(const float logit[9], uint32_t allowed, int mode, float u, float& logp) {
  int first = 0, last = 0;
  bool any = false;
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < MLP_OUT; ++k)
    if ((allowed >> k) & 1u) {
      if (!any) first = k, m = logit[k];
      m = logit[k] > m ? logit[k] : m;
      any = true;
      last = k;
    }
  float e[MLP_OUT];
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < MLP_OUT; ++k) {
    e[k] = 0.0f;
    if ((allowed >> k) & 1u) {
      e[k] = expf(logit[k] - m);
      z = z + e[k];
    }
  }
  int a;
  if (mode == MLP_GREEDY) {
    a = first;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < MLP_OUT; ++k)
      if (((allowed >> k) & 1u) && !hit && logit[k] == m) a = k, hit = true;
  } else {
    const float thr = u * z;
    a = last;
    bool hit = false;
    float run = 0.0f;
#pragma unroll
    for (int k = 0; k < MLP_OUT; ++k)
      if ((allowed >> k) & 1u) {
        run = run + e[k];
        if (!hit && run > thr) a = k, hit = true;
      }
  }
  float la = logit[0];
#pragma unroll
  for (int k = 1; k < MLP_OUT; ++k) la = (a == k) ? logit[k] : la;
  logp = (la - m) - logf(z);
  return a;
}

}  // namespace tg
