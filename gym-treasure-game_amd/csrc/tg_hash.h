// tg_hash.h — sm64, the splitmix64 finaliser every synthetic stream is built from: the synthetic
// policies' actions (tg_rules.h policy_action), the learned actor's sampling uniform
// (tg_policy_mlp.h mlp_uniform) and the host checks' record hash.  The one copy.  Stand-alone:
// <stdint.h> only, so the plain-g++ build of tg_policy_mlp.h (tests/native_policy) can include it;
// under hipcc it is `__host__ __device__` like the rest of the per-env core (tg_state.h's TG_HD).
#pragma once
#include <stdint.h>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif
#ifndef TG_HD
#ifdef __HIP__
#define TG_HD __host__ __device__ __forceinline__  // tg_state.h's
#else
#define TG_HD inline
#endif
#endif

namespace tg {

TG_HD uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace tg
