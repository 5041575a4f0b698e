// tg_hostcheck_policy.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the learned actor's arithmetic (gym-treasure-game_amd/csrc/tg_policy_mlp.h),
// exported over arrays: the same functions k_policy_mlp evaluates per lane, so the tests can
// hold the device's logits and values to these bit for bit and check both against an
// independent float64 evaluation.  What the kernel adds around them (the state unpack, the obs
// row, available_mask, the stores) is covered by tests/test_gpu_policy_mlp.py.  The product
// library never contains or calls this.  Built by tests/native_policy/Makefile with g++ and
// -ffp-contract=off.
#include <cstdint>

#include "../../gym-treasure-game_amd/csrc/tg_policy_mlp.h"

using namespace tg;

namespace {
template <int H>
void forward_rows(int act, const float* p, const double* obs, int64_t n, float* logits,
                  float* value) {
  for (int64_t i = 0; i < n; ++i) {
    if (act == MLP_ACT_RELU)
      mlp_forward<H, MLP_ACT_RELU>(p, obs + 9 * i, logits + 9 * i, value[i]);
    else if (act == MLP_ACT_TANH)
      mlp_forward<H, MLP_ACT_TANH>(p, obs + 9 * i, logits + 9 * i, value[i]);
    else
      mlp_forward<H, MLP_ACT_TANH_F64>(p, obs + 9 * i, logits + 9 * i, value[i]);
  }
}
}  // namespace

extern "C" {

int pm_param_count(int hidden) { return mlp_hidden_ok(hidden) ? mlp_param_count(hidden) : -1; }

// logits [n][9] and value [n] of the obs rows [n][9] (f64).  act: 0 relu, 1 tanhf, 2 the double
// library's tanh rounded to f32.  Returns -1 for a bad hidden width or act.
int pm_forward(int hidden, int act, const float* params, const double* obs, int64_t n,
               float* logits, float* value) {
  if (act < 0 || act > 2) return -1;
  switch (hidden) {
    case 16: forward_rows<16>(act, params, obs, n, logits, value); return 0;
    case 32: forward_rows<32>(act, params, obs, n, logits, value); return 0;
    case 64: forward_rows<64>(act, params, obs, n, logits, value); return 0;
    case 128: forward_rows<128>(act, params, obs, n, logits, value); return 0;
  }
  return -1;
}

// u of (action seed, global env g0 + i, step t) for i < n
void pm_uniform(uint64_t a0, int64_t g0, int64_t t, int64_t n, float* u) {
  for (int64_t i = 0; i < n; ++i) u[i] = mlp_uniform(a0, g0 + i, t);
}

// actions and logp of logits [n][9] with available_mask bits avail [n] (u16), env i being the
// global env g0 + i at step t.  mode: 0 sample, 1 greedy.
void pm_select(const float* logits, const uint16_t* avail, int masked, int mode, uint64_t a0,
               int64_t g0, int64_t t, int64_t n, int32_t* actions, float* logp) {
  for (int64_t i = 0; i < n; ++i)
    actions[i] = mlp_select(logits + 9 * i, mlp_allowed(masked, avail[i]), mode,
                            mlp_uniform(a0, g0 + i, t), logp[i]);
}

}  // extern "C"
