// tg_run_diag.h — k_run's per-wave timing, for the DIAGNOSTIC build -DTG_DIAG_STAMPS only
// (scripts/diag_stamps.py builds it and reads the record through tg_diag_stamps, tg_amd.hip).
// tg_dev.h includes this header; without the macro RunPhaseClock and RunStamp are empty types
// whose members do nothing, so RngCodesT::phase and k_run's hook calls compile to no code and
// the product holds no stamp.  With it:
//   RunPhaseClock  a lane's s_memtime sums per phase of its option loop (RngCodesT::phase feeds
//                  it from tg_core.h's counted_tick / span_loop)
//   RunStamp       a wave's stamps in k_run: begin, envs loaded, option done, end of wave
//   g_stamps       the record, NSTAMP words per wave:
//                    0 load, 1 option loop, 2 epilogue (s_memtime cycles of the first live lane;
//                      an idle wave: 0, 0, its whole time)
//                    3 max ticks | sum of ticks << 32 | option << 56 (an idle wave, one without a
//                      listed chunk: option 15 with 1 iteration)
//                    4 start, 5 end (s_memrealtime: 100 MHz, chip-wide)
//                    6 plain walk, 7 window refill, 8 full ticks, 9 rounds: the phase clock of the
//                      lane whose option loop ran longest (the wave's own time)
//                    10 the halves an idle wave regenerated in k_run's quiet drain (else 0)
#pragma once

namespace {  // as the rest of the device layer: each unit its own

#ifdef TG_DIAG_STAMPS
constexpr int NSTAMP = 11;
constexpr int NSTAMP_WAVES = 1 << 17;
__device__ unsigned long long g_stamps[NSTAMP_WAVES * NSTAMP];

struct RunPhaseClock {
  // ph[k] sums the time of the segments ending at mark k (1 plain walk, 2 window refill,
  // 3 full tick); rounds counts mark 0
  unsigned long long ph[4] = {0, 0, 0, 0}, last = 0;
  uint32_t rounds = 0;
  __device__ __forceinline__ void mark(int k) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    if (last) ph[k] += now - last;
    last = now;
    rounds += k == 0;
  }
};

struct RunStamp {
  unsigned long long t0 = 0, t1 = 0, t2 = 0, rt0 = 0;
  unsigned long long ph1 = 0, ph2 = 0, ph3 = 0;
  uint32_t rounds = 0;
  __device__ __forceinline__ void begin() {
    t0 = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
  }
  __device__ __forceinline__ void env_loaded() { t1 = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void option_done(const RunPhaseClock& c) {
    t2 = __builtin_amdgcn_s_memtime();
    ph1 = c.ph[1], ph2 = c.ph[2], ph3 = c.ph[3], rounds = c.rounds;
  }
  // wv: the wave's index in the grid; k: its option (wave-uniform); ticks: this lane's
  // halves: an idle wave's quiet drain's
  __device__ __forceinline__ void wave_end(bool live, int k, int ticks, int wv, int halves = 0) const {
    const unsigned long long t3 = __builtin_amdgcn_s_memtime();
    int mx = ticks, sum = ticks;
    for (int o = 32; o > 0; o >>= 1) {
      mx = max(mx, __shfl_xor(mx, o, 64));
      sum += __shfl_xor(sum, o, 64);
    }
    const unsigned long long bl = __ballot(live);
    const int src = bl ? __ffsll((long long)bl) - 1 : 0;
    const unsigned long long a1 = __shfl(t1, src, 64);
    const unsigned long long a2 = __shfl(t2, src, 64);
    const unsigned long long rt3 = __builtin_amdgcn_s_memrealtime();
    int lmax = src;
    unsigned long long best = 0;
    for (int l = 0; l < 64; ++l) {
      const unsigned long long tl = __shfl(ph1 + ph2 + ph3, l, 64);
      if (((bl >> l) & 1ull) && tl > best) best = tl, lmax = l;
    }
    const unsigned long long p1 = __shfl(ph1, lmax, 64), p2 = __shfl(ph2, lmax, 64),
                             p3 = __shfl(ph3, lmax, 64);
    const uint32_t pr = __shfl(rounds, lmax, 64);
    if ((threadIdx.x & 63) == 0 && wv < NSTAMP_WAVES) {
      unsigned long long* const g = g_stamps + (size_t)wv * NSTAMP;
      g[0] = bl ? a1 - t0 : 0;
      g[1] = bl ? a2 - a1 : 0;
      g[2] = bl ? t3 - a2 : t3 - t0;
      g[3] = bl ? (unsigned long long)mx | ((unsigned long long)sum << 32) | ((unsigned long long)k << 56)
                : 1ull | (15ull << 56);
      g[4] = rt0;
      g[5] = rt3;
      g[6] = p1;
      g[7] = p2;
      g[8] = p3;
      g[9] = pr;
      g[10] = (unsigned long long)halves;
    }
  }
};
#else
struct RunPhaseClock {
  __device__ __forceinline__ void mark(int) {}
};
struct RunStamp {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void env_loaded() {}
  __device__ __forceinline__ void option_done(const RunPhaseClock&) {}
  __device__ __forceinline__ void wave_end(bool, int, int, int, int = 0) const {}
};
#endif
// run_listed's hook where nothing is stamped (k_flow), in every build
struct NoRunHook {
  __device__ __forceinline__ void env_loaded() {}
  __device__ __forceinline__ void option_done(const RunPhaseClock&) {}
};

}  // namespace
