// tg_value_mlp.h — the learned actor's value alone, over a range of envs or over a device list of
// saved states (tg_rollout_mlp_gae): k_value_mlp, and k_trunc_list, which saves the
// states of the envs k_timelimit is about to reset.  Compiled by tg_amd.hip only.
//
// In a rollout with a step limit and auto-reset, launch_step runs k_trunc_list between a step's
// kernels and k_timelimit: the envs' states are still the ones the step left, and the list gets
// each truncated env's 32 B of state and where its value belongs in the rollout's vnext rows.
// Nothing else waits on the step's stream: k_value_mlp runs over the list once, after the
// rollout's last step (or earlier, when the list's bound is reached), and stores each value by
// its destination.  The list's order follows the workgroups' atomics and is not deterministic;
// what is stored does not depend on it.
#pragma once
#include "tg_dev.h"
#include "tg_policy_mlp.h"

namespace {

constexpr int TL_BLOCK = 1024, TL_TILES = 4;  // k_trunc_list: envs per workgroup = 4,096

// the list: entry k is an env's state words as S holds them and its destination, the index into
// the rollout's vnext rows; cap entries
struct TruncList {
  uint4* st4;
  double2* ang;
  int64_t* dst;
  int64_t cap;
};

// envs [0, n) of the view S after step `tstep`: those k_timelimit will find truncated (its
// predicate on the same episode word), appended to T at *cur; env i's destination is dst0 + i.
// The slots are reserved per workgroup of TL_TILES x TL_BLOCK envs (the waves' counts through
// LDS, one atomic: tg_timelimit.h says why not per wave; 256 atomics per step at 1M envs).
// *nxt, the count of the list's other use, is zeroed (the k_value_mlp that read it has finished).
__global__ __launch_bounds__(TL_BLOCK) void k_trunc_list(Soa S, int64_t n, uint32_t limit, uint32_t tstep,
                                                          int64_t dst0, TruncList T, int32_t* cur,
                                                          int32_t* nxt) {
  constexpr int WAVES = TL_BLOCK / 64;
  __shared__ int wcnt[TL_TILES * WAVES], bbase;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * (TL_TILES * TL_BLOCK) + threadIdx.x;
  if (i0 == 0) *nxt = 0;
  unsigned long long tb[TL_TILES];
  bool trunc[TL_TILES];
#pragma unroll
  for (int j = 0; j < TL_TILES; ++j) {
    const int64_t i = i0 + j * TL_BLOCK;
    trunc[j] = i < n && tstep + 1u - (uint32_t)S.ep[i].y >= limit;
    tb[j] = __ballot(trunc[j]);
    if (lane == 0) wcnt[j * WAVES + wave] = __popcll(tb[j]);
  }
  __syncthreads();
  int cnt = 0, before[TL_TILES];
#pragma unroll
  for (int j = 0; j < TL_TILES; ++j) {
    before[j] = 0;
    for (int v = 0; v < WAVES; ++v) {
      if (v == wave) before[j] = cnt;
      cnt += wcnt[j * WAVES + v];
    }
  }
  if (!cnt) return;  // workgroup-uniform
  if (threadIdx.x == 0) bbase = atomicAdd(cur, cnt);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TL_TILES; ++j)
    if (trunc[j]) {
      const int64_t i = i0 + j * TL_BLOCK;
      const int64_t slot = (int64_t)bbase + before[j] + __popcll(tb[j] & ((1ull << lane) - 1ull));
      if (slot >= 0 && slot < T.cap) {  // (the host's bound on the list keeps every slot inside)
        T.st4[slot] = S.st4[i];
        T.ang[slot] = S.ang[i];
        T.dst[slot] = dst0 + i;
      }
    }
}

// The value tg_policy_mlp computes for a state (the same tg::mlp_forward on the same observe row):
//   T.st4 null: of envs [0, n) of the view S, value[i];
//   else: of the list's entries k < min(*count, T.cap), value[T.dst[k]] where that lies in
//   [0, total); S and n are not used.
// The list form's grid covers the host's bound on the count: a workgroup past the count leaves
// after one scalar load.  No masks, no sampling, no atomics.
template <int H, int ACT>
__global__ __launch_bounds__(BLOCK) void k_value_mlp(Soa S, int64_t n, Level L,
                                                      const float* __restrict__ params, TruncList T,
                                                      const int32_t* __restrict__ count,
                                                      float* __restrict__ value, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t dst = i;
  uint4 st4;
  double2 ang;
  if (T.st4) {
    int64_t c = *count;
    c = c < T.cap ? c : T.cap;
    if ((int64_t)blockIdx.x * BLOCK >= c) return;
    if (i >= c) return;
    dst = T.dst[i];
    if (dst < 0 || dst >= total) return;
    st4 = T.st4[i];
    ang = T.ang[i];
  } else {
    if (i >= n) return;
    st4 = S.st4[i];
    ang = S.ang[i];
  }
  Env e;
  unpack(st4, ang, e);
  double o[9];
  observe(L, e, o);
  float lg[MLP_OUT], v;
  mlp_forward<H, ACT>(params, o, lg, v);
  value[dst] = v;
}

}  // namespace
