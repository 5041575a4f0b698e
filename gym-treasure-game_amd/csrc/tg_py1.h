// tg_py1.h — the N = 1 path's kernels: k_py1 (one call over a Python-level random stream) and
// k_serve1 (the resident server).  Compiled by tg_amd.hip only, whose host code launches them.
#pragma once
#include "tg_dev.h"

namespace {

// ---- the N=1 drop-in over a Python-level random stream (tg_step1_py / tg_reset1_py) ---------
// One wave.  The stream's generation (tg_pystate: random.getstate()'s 624 words + index) is read
// from pinned host memory into LDS with its two successors (twisted by the wave), lane 0 runs the
// step / reset with a PyRng over them, and the wave writes back the generation holding the
// stream's new position, so the caller's random.setstate continues exactly where CPython's
// would: any index, odd ones too (the twist is a recurrence on consecutive words, so words are
// read by absolute position across generations), and gauss_next carried in and out.
constexpr int PY_GENS = 3;  // generations held in LDS; a 4th+ is twisted in place by lane 0
struct PyRng {
  uint32_t* w;     // LDS: PY_GENS slots of MT_N words, generation g in slot (g + off) % PY_GENS
  uint32_t q;      // absolute word position (generation g holds positions [g*624, g*624 + 624))
  uint32_t lo;     // oldest generation held
  uint32_t draws;
  uint32_t off;    // the ring's rotation (k_serve1 keeps the ring in LDS across calls)
  // the generation holding the next word, its slot and the word's index there (set up at the
  // first draw; a draw crosses into the next generation only every 312 draws)
  uint32_t gc = 0u, qi = 0u;
  const uint32_t* cs = nullptr;
  __device__ __forceinline__ uint32_t* slot(uint32_t g) const { return w + ((g + off) % PY_GENS) * MT_N; }
  __device__ __forceinline__ const uint32_t* gen(uint32_t g) {
    while (g >= lo + PY_GENS) {  // > 2 generations in one call (long levels): twist in place
      twist_gen(slot(lo + PY_GENS - 1), slot(lo));
      ++lo;
    }
    return slot(g);
  }
  __device__ __forceinline__ uint32_t next_word() {
    if (qi == (uint32_t)MT_N) {
      cs = gen(++gc);
      qi = 0u;
    }
    return cs[qi++];
  }
  __device__ __forceinline__ double random() {
    if (!cs) {
      gc = q / MT_N;
      qi = q - gc * MT_N;
      cs = gen(gc);
    }
    uint32_t a, b;
    if (qi + 2u <= (uint32_t)MT_N) {  // both words in the current generation
      a = cs[qi];
      b = cs[qi + 1u];
      qi += 2u;
    } else {
      a = next_word();
      b = next_word();
    }
    q += 2;
    ++draws;
    return mt_double(a, b);
  }
  __device__ __forceinline__ double uniform(double a, double b) { return a + (b - a) * random(); }
  __device__ __forceinline__ uint32_t code() { return draw_code(random()); }
  __device__ __forceinline__ void reserve(uint32_t) {}
  __device__ __forceinline__ bool has(uint32_t) const { return true; }
  __device__ __forceinline__ bool overrun() const { return false; }
  __device__ __forceinline__ void phase(int) {}
  template <int DIR>
  __device__ __forceinline__ int walk(int& x, int lim, int cap) { return walk_ticks<DIR>(*this, x, lim, cap); }
};
// dst = twist_gen(src) with the 64 lanes of the (only) wave, both in LDS
__device__ __forceinline__ void lds_twist64(const uint32_t* src, uint32_t* dst) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int r = 0; r < (MT_N + 63) / 64; ++r) {
    const int p = r * 64 + lane;
    if (p < MT_N) {
      const uint32_t b = p + 1 < MT_N ? src[p + 1] : dst[0];
      const uint32_t c = p < MT_N - MT_M ? src[p + MT_M] : dst[p - (MT_N - MT_M)];
      dst[p] = mt_twist(src[p], b, c);
    }
    __syncthreads();
  }
}
// lane 0 runs the call (a step of `action`, or RESET) over the ring W, where generation j of the
// caller's stream (j = 0: the one tg_pystate holds; q0 its index) sits in slot (j + off) % 3.
// On return py holds the state after the call: its index and gauss_next, and the generation's
// words when the generation changed (otherwise py's words already are the generation's); the
// ring holds the new generation and its two successors, off updated to match.  Returns the new
// generation's number (0: unchanged).  Every lane of the (one-wave) workgroup must reach it.
template <bool RESET>
__device__ __forceinline__ uint32_t py_call(const Soa& S, const Level& L, const LdsLevel& lv,
                                            uint32_t* W, uint32_t& off, int action,
                                            tg_pystate* py, uint32_t q0, int has_gauss,
                                            double gauss_next, TgOne* out, uint32_t tstep,
                                            unsigned long long* __restrict__ stats,
                                            uint32_t* __restrict__ err_or, int* ticks = nullptr,
                                            const uint32_t* mk = nullptr,
                                            unsigned long long* stamps = nullptr) {
  __shared__ uint32_t out_g, out_lo, out_idx;
  const int lane = threadIdx.x;
  StepResult r{0, 0, 0, 0};
  uint32_t draws = 0;
  if (lane == 0) {
    const Map m{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H, mk};
    PyRng rng{W, q0, 0u, 0u, off};
    Env e;
    unpack(S.st4[0], S.ang[0], e);
    int2 ep = S.ep[0];
    double o[9];
    if (stamps) stamps[0] = __builtin_amdgcn_s_memrealtime();
    if (RESET) {
      GaussNext g{has_gauss != 0, gauss_next};
      reset_env_gauss(L, e, rng, g);
      py->has_gauss = g.has ? 1u : 0u;
      py->gauss_next = g.has ? g.v : 0.0;
      ep = make_int2(0, (int32_t)tstep);  // the episode starts with the next step
    } else {
      r = env_step(L, lv.trig, m, e, action, rng);
      ep.x += r.reward;  // (ep.y: the episode's start step)
    }
    if (stamps) stamps[1] = __builtin_amdgcn_s_memrealtime();
    observe(level_div(L), e, o);  // by f64 division, as k_run (the table's loads: 0.48 us)
    if (stamps) stamps[2] = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int k = 0; k < 9; ++k) out->obs[k] = o[k];
    out->reward = r.reward;
    out->valid = (uint8_t)r.ran;
    out->done = (uint8_t)r.done;
    S.st4[0] = pack(e);
    S.ang[0] = make_double2(e.ang0, e.ang1);
    S.ep[0] = ep;
    if (e.f & E_MASK) atomicOr(err_or, e.f & E_MASK);
    // CPython's state after the last word read: its generation and the index past it
    const uint32_t g = rng.q == q0 ? 0u : (rng.q - 1u) / MT_N;
    out_g = g;
    out_lo = rng.lo;
    out_idx = rng.q == q0 ? q0 : rng.q - g * MT_N;
    draws = rng.draws;
  }
  __syncthreads();
  if (stamps && lane == 0) stamps[3] = __builtin_amdgcn_s_memrealtime();
  const uint32_t g = out_g;
  if (g != 0u) {  // the caller's generation changed
    const uint32_t* src = W + ((g + off) % PY_GENS) * MT_N;
    for (int i = lane; i < MT_N; i += 64) py->mt[i] = src[i];
    // the ring: generations g, g + 1, g + 2 (it holds out_lo .. out_lo + 2, g among them; the
    // missing successors are twisted over generations older than g)
    for (uint32_t hi = out_lo + PY_GENS - 1; hi < g + PY_GENS - 1; ++hi)
      lds_twist64(W + ((hi + off) % PY_GENS) * MT_N, W + ((hi + 1 + off) % PY_GENS) * MT_N);
    off = (off + g) % PY_GENS;
  }
  if (lane == 0) py->index = out_idx;
  lane0_stats(stats, !RESET ? 1 : 0, r.ran, r.ticks, (int)draws, 0);
  if (ticks) *ticks = r.ticks;
  if (stamps && lane == 0) stamps[4] = __builtin_amdgcn_s_memrealtime();
  return g;
}
// the ring from the caller's state (py, pinned host memory): its generation and two successors
__device__ __forceinline__ void py_ring_cold(uint32_t* W, const tg_pystate* py) {
  for (int i = threadIdx.x; i < MT_N; i += 64) W[i] = py->mt[i];
  __syncthreads();
  lds_twist64(W, W + MT_N);
  lds_twist64(W + MT_N, W + 2 * MT_N);
}
// The Python stream's generation and its two successors, kept on the device between calls
// (tg_batch::pyc, generation j in slot j): cache_in is it when the caller's state is the one the
// last call returned (the host compares them), else null and the ring is built from the
// caller's state.  q0 / gauss: the caller's index and gauss_next, as kernel arguments (no
// host-memory reads in the common case).  On return py holds the state after the call and
// cache_out the new generation and its two successors.
template <bool RESET>
__global__ __launch_bounds__(64) void k_py1(Soa S, Level L, const uint32_t* __restrict__ grid,
                                            int action, tg_pystate* py, const uint32_t* cache_in,
                                            uint32_t* cache_out, uint32_t q0, int has_gauss,
                                            double gauss_next, TgOne* out, uint32_t tstep,
                                            unsigned long long* __restrict__ stats,
                                            uint32_t* __restrict__ err_or) {
  __shared__ uint32_t W[PY_GENS * MT_N];
  __shared__ LdsLevel lv;
  const int lane = threadIdx.x;
  stage_cells<64>(lv.grid, lv.trig, grid, L);
  if (cache_in) {
    for (int i = lane; i < PY_GENS * MT_N; i += 64) W[i] = cache_in[i];
    __syncthreads();
  } else {
    py_ring_cold(W, py);
  }
  uint32_t off = 0;
  const uint32_t g = py_call<RESET>(S, L, lv, W, off, action, py, q0, has_gauss, gauss_next, out,
                                    tstep, stats, err_or);
  if (g != 0u || !cache_in)
    for (int j = 0; j < PY_GENS; ++j)
      for (int i = lane; i < MT_N; i += 64) cache_out[j * MT_N + i] = W[((j + off) % PY_GENS) * MT_N + i];
}

// ---- the N = 1 server (tg_batch::serve) ------------------------------------------------------
// One wave, resident for a 1-env handle's tg_step1 / tg_step1_py / tg_step1_pywords /
// tg_reset1_py / tg_available_mask1: it polls the
// mailbox's seq (a system-scope load of pinned host memory), serves a new command with the same
// device code as k_step<POL_IMMEDIATE> / k_py1 (step_env, py_call), writes the result row and
// the stream state into pinned host memory, releases them at system scope and then stores
// done = seq, which the host spins on.  The level, the env's state and the Python stream's ring
// (rotated by off) stay in LDS between commands (the private stream's code window is primed
// afresh by each step, as in k_step).  Every lane leaves together, on SRV_QUIT or
// after `idle` ticks of s_memrealtime (100 MHz) without a command; a leaving server writes the
// ring to pyc (generation j in slot j), where the next server or k_py1 finds it.
__device__ __forceinline__ uint32_t sys_load(const uint32_t* p) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
// Resident for many commands, the server keeps in LDS what a step would otherwise fetch from
// HBM each time: the env's state (st4 / ang / ep: written back to HBM when it leaves), the level
// bitmasks and, when it fits (`stage`: dynamic LDS, sized at launch), the GoTable.  (get_state
// divides, as k_run: no quotient table.)
constexpr uint32_t SRV_STAGE_GOTAB = 1u;
__global__ __launch_bounds__(64) void k_serve1(Soa Sg, Level Lg, const uint32_t* __restrict__ grid,
                                               SrvBox* box, tg_pystate* py, uint32_t* pyc,
                                               TgOne* out, EpQueue q, int64_t g0, uint32_t idle,
                                               int trace, uint32_t stage,
                                               unsigned long long* __restrict__ stats,
                                               uint32_t* __restrict__ err_or) {
  __shared__ __attribute__((aligned(16))) uint8_t win[WIN_WAVE_BYTES];
  __shared__ uint32_t W[PY_GENS * MT_N];
  __shared__ LdsLevel lv;
  __shared__ uint4 st4_l;
  __shared__ double2 ang_l;
  __shared__ int2 ep_l;
  __shared__ uint32_t mk_l[MK_MAX_WORDS];  // the level bitmasks (Map::mk), as k_run's
  extern __shared__ __attribute__((aligned(16))) uint8_t srv_dyn[];
  const int lane = threadIdx.x;
  stage_cells<64>(lv.grid, lv.trig, grid, Lg, mk_l);
  const uint32_t* const mk = Lg.masks ? mk_l : nullptr;
  Level L = Lg;
  if (stage & SRV_STAGE_GOTAB) {
    uint32_t* const gd = reinterpret_cast<uint32_t*>(srv_dyn);
    const int ng = Lg.W * Lg.H * 32;
    for (int i = lane; i < ng; i += 64) gd[i] = Lg.gotab[i];
    L.gotab = gd;
  }
  if (lane == 0) {
    st4_l = Sg.st4[0];
    ang_l = Sg.ang[0];
    ep_l = Sg.ep[0];
  }
  __syncthreads();
  const Soa S{&st4_l, &ang_l, &ep_l, Sg.mt, Sg.mc};
  const Map m{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H, mk};
  bool ring = false;  // W holds the Python stream's ring
  uint32_t off = 0;
  uint32_t served = sys_load(&box->done);
  unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
  __shared__ TgOne row_l;  // the command's result row, written to host memory in one burst
  __shared__ unsigned long long phase_l[5];  // TG_SERVE_TRACE: py_call's phase stamps
  TgOne* const row = &row_l;
  while (true) {
    // the command group in one load (volatile: system scope, no cache)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 cg = *reinterpret_cast<const volatile u32x4*>(box);
    const uint32_t s = __builtin_amdgcn_readfirstlane(cg.w);
    if (s == served) {
      if (__builtin_amdgcn_s_memrealtime() - t_last > idle) break;
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // what the host wrote before seq
    const unsigned long long t_seen = __builtin_amdgcn_s_memrealtime();
    int ticks = 0;
    const uint32_t word = __builtin_amdgcn_readfirstlane(cg.x);
    const uint32_t kind = srv_kind(word);  // (tg_srv_word.h, beside the host's encoder)
    if (kind == SRV_QUIT) {
      served = s;
      break;
    }
    const int action = srv_action(word);  // an action out of range arrives as one (-16)
    const uint32_t tstep = __builtin_amdgcn_readfirstlane(cg.y);
    if (kind == SRV_MASK) {  // available_mask (TG/:83-89), as k_mask
      if (lane == 0) {
        Env e;
        unpack(S.st4[0], S.ang[0], e);
        box->mask = available_mask(L, m, e);
      }
    } else if (kind == SRV_RESET) {  // reset() on the env's own stream, as k_reset
      Env e;
      e.mti = 0u;
      if (lane == 0) {
        unpack(S.st4[0], S.ang[0], e);
        Rng rng(S.mt, e.mti, S.mc);
        reset_env(L, e, rng);
        e.mti = rng.finish();
        double o[9];
        observe(level_div(L), e, o);
#pragma unroll
        for (int k = 0; k < 9; ++k) row->obs[k] = o[k];
        row->reward = 0;
        row->valid = 0;
        row->done = 0;
      }
      wave_refill(__ballot(lane == 0 && (e.mti & MT_STALE)), S.mt, S.mc, e.mti, (lds_u32*)win);
      if (lane == 0) {
        e.mti &= ~(MT_STALE | MT_LISTED);
        S.st4[0] = pack(e);
        S.ang[0] = make_double2(e.ang0, e.ang1);
        S.ep[0] = make_int2(0, (int32_t)tstep);  // the episode starts with the next step
      }
    } else if (kind == SRV_STEP) {
      const StepIO io{nullptr, row->obs, &row->reward, &row->valid, &row->done, nullptr,
                      POL_IMMEDIATE, (uint64_t)(int64_t)action, 0, tstep};
      ticks = step_env<false, false, POL_IMMEDIATE, true>(S, 1, L, lv.trig, m, (lds_u8*)win, lane, io,
                                                          q, g0, stats, err_or).ticks;
    } else {
      const bool warm = srv_warm(word);
      const int has_gauss = (int)srv_has_gauss(word);
      const uint32_t q0 = srv_q0(word);
      double gauss_next = 0.0;
      if (kind == SRV_RESET_PY) {
        const uint32_t* gp = reinterpret_cast<const uint32_t*>(&box->gauss_bits);
        gauss_next = __builtin_bit_cast(double, (uint64_t)sys_load(gp) | (uint64_t)sys_load(gp + 1) << 32);
      }
      if (!ring || !warm) {  // a new server, or draws on the stream since the last call
        if (warm) {
          for (int i = lane; i < PY_GENS * MT_N; i += 64) W[i] = pyc[i];
          __syncthreads();
        } else {
          py_ring_cold(W, py);
        }
        off = 0;
        ring = true;
      }
      if (kind == SRV_RESET_PY)
        py_call<true>(S, L, lv, W, off, 0, py, q0, has_gauss, gauss_next, row, tstep, stats, err_or,
                      &ticks, mk);
      else
        py_call<false>(S, L, lv, W, off, action, py, q0, has_gauss, gauss_next, row, tstep, stats,
                       err_or, &ticks, mk, trace ? phase_l : nullptr);
    }
    __syncthreads();
    if (kind != SRV_MASK && lane < (int)(sizeof(TgOne) / 8))
      reinterpret_cast<uint64_t*>(out)[lane] = reinterpret_cast<const uint64_t*>(row)[lane];
    // the row and the state (host memory; the env's state and MT ring in HBM for the next
    // command) before the answer
    if (trace && lane == 0) {
      box->t_seen = t_seen;
      box->t_end = __builtin_amdgcn_s_memrealtime();
      box->ticks = (uint32_t)ticks;
      for (int j = 0; j < 5; ++j) box->phase[j] = kind == SRV_STEP_PY ? phase_l[j] : 0ull;
    }
    __syncthreads();  // (the release below covers the row the lanes wrote: one wave)
    if (lane == 0) __hip_atomic_store(&box->done, s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    served = s;
    t_last = __builtin_amdgcn_s_memrealtime();
  }
  if (ring)
    for (int j = 0; j < PY_GENS; ++j)
      for (int i = lane; i < MT_N; i += 64) pyc[j * MT_N + i] = W[((j + off) % PY_GENS) * MT_N + i];
  __syncthreads();
  if (lane == 0) {
    Sg.st4[0] = st4_l;
    Sg.ang[0] = ang_l;
    Sg.ep[0] = ep_l;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __syncthreads();
  if (lane == 0) __hip_atomic_store(&box->done, served, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace
