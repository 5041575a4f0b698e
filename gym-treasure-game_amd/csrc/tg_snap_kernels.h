// tg_snap_kernels.h — the snapshot kernels (tg_snap_save / tg_snap_load, include/tg_amd.h): envs
// to slots and slots to envs through device index lists, one slot as tg_snapshot.h defines it.
// Compiled by tg_amd.hip only, whose host code launches them.  Both are HBM streams: a save reads
// one generation (2,496 B; an odd one is twisted from the stored one before it) and writes a
// slot, 2,536 B; a load reads a slot and writes the env's ring, 8 stored generations and 16
// generations of codes, 24,960 B.  Every address comes from an index checked against its array.
#pragma once
#include "tg_dev.h"
#include "tg_snapshot.h"

namespace {

constexpr uint32_t E_INDEX = TG_ERR_INDEX;  // handle-level: never in an env's flag word

// an entry's env and slot, or false (and TG_ERR_INDEX, once per entry: `report`)
__device__ __forceinline__ bool snap_entry(const int64_t* __restrict__ envs,
                                           const int64_t* __restrict__ slots, int64_t k, int64_t n,
                                           int64_t nslots, bool report, uint32_t* err, int64_t& env,
                                           int64_t& slot) {
  env = envs[k];
  slot = slots[k];
  const bool ok = (uint64_t)env < (uint64_t)n && (uint64_t)slot < (uint64_t)nslots;
  if (!ok && report) atomicOr(err, E_INDEX);
  return ok;
}

// slot slots[k] <- env envs[k]: one lane per 16 B of the generation (SNAP_Q lanes per entry;
// lane 0 of an entry also moves the three small words), 16-B coalesced stores
__global__ __launch_bounds__(BLOCK) void k_snap_save(Soa S, int64_t n, Snap P, int64_t nslots,
                                                      const int64_t* __restrict__ envs,
                                                      const int64_t* __restrict__ slots, int64_t count,
                                                      uint32_t tstep, uint32_t* __restrict__ err) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= count * SNAP_Q) return;
  const int64_t k = t / SNAP_Q;
  const int q = (int)(t - k * SNAP_Q);
  int64_t env, slot;
  if (!snap_entry(envs, slots, k, n, nslots, q == 0, err, env, slot)) return;
  const uint4 st = S.st4[env];
  reinterpret_cast<uint4*>(P.mt + slot * MT_N)[q] = snap_gen_quad(S.mt + env * MT_STORE, snap_gen(st.w), q);
  if (q == 0) {
    P.st4[slot] = snap_pack_st4(st);
    P.ang[slot] = S.ang[env];
    P.ep[slot] = snap_pack_ep(S.ep[env], tstep);
  }
}

// tg_snap_load's seeds: random.seed(seeds[k]) of env envs[k], init_by_array into half 0's last
// stored slot as k_create, one env per lane (seed_mt is a dependent chain); k_snap_load<true>
// makes the ring from it.  (A bad entry is k_snap_load's to report.)
__global__ __launch_bounds__(BLOCK) void k_snap_seed(Soa S, int64_t n, int64_t nslots,
                                                      const int64_t* __restrict__ envs,
                                                      const int64_t* __restrict__ slots,
                                                      const uint64_t* __restrict__ seeds, int64_t count,
                                                      const uint32_t* __restrict__ genrand) {
  const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  int64_t env, slot;
  if (!snap_entry(envs, slots, k, n, nslots, false, nullptr, env, slot)) return;
  seed_mt(S.mt + env * MT_STORE + MT_SEED_OFF, genrand, seeds[k]);
}

// env envs[k] <- slot slots[k], one wavefront per entry: the state words (lane 0), the slot's
// generation into ring generation 0 with its codes (each lane 16 B of words and their two codes),
// then the 15 successors by wave_twist_gens, whose source is the slot's copy of the generation
// (the same words as ring generation 0, and nothing this launch writes).  SEEDED: the game state
// alone is the slot's; the ring is the 16 generations after the words k_snap_seed left, position
// 0, as tg_create.
template <bool SEEDED>
__global__ __launch_bounds__(BLOCK) void k_snap_load(Soa S, int64_t n, Snap P, int64_t nslots,
                                                      const int64_t* __restrict__ slots,
                                                      const int64_t* __restrict__ envs, int64_t count,
                                                      uint32_t tstep, uint32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) uint32_t scratch[BLOCK / 64][MT_N];
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);  // wave-uniform
  if (k >= count) return;
  int64_t env, slot;
  if (!snap_entry(envs, slots, k, n, nslots, lane == 0, err, env, slot)) return;
  uint32_t* const mt = S.mt + env * MT_STORE;
  uint8_t* const mc = S.mc + env * MT_CODES;
  const uint32_t* const gen = P.mt + slot * MT_N;
  if (lane == 0) {
    S.st4[env] = snap_unpack_st4(P.st4[slot], SEEDED);
    S.ang[env] = P.ang[slot];
    S.ep[env] = snap_unpack_ep(P.ep[slot], tstep);
  }
  lds_u32* const scr = (lds_u32*)scratch[threadIdx.x >> 6];
  if constexpr (SEEDED) {
    wave_twist_gens((const glb_u32*)(mt + MT_SEED_OFF), (glb_u32*)mt, mc, 0, 2 * MT_HALF_GENS, false, scr);
  } else {
#pragma unroll
    for (int r = 0; r < (SNAP_Q + 63) / 64; ++r) {
      const int q = r * 64 + lane;
      if (q < SNAP_Q) {
        const uint4 v = reinterpret_cast<const uint4*>(gen)[q];
        reinterpret_cast<uint4*>(mt)[q] = v;
        reinterpret_cast<uint16_t*>(mc)[q] = (uint16_t)snap_quad_codes(v);
      }
    }
    wave_twist_gens((const glb_u32*)gen, (glb_u32*)mt, mc, 1, 2 * MT_HALF_GENS - 1, false, scr);
  }
}

}  // namespace
