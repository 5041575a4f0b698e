// tg_dev.h — the device layer both device units of the step code compile: tg_amd.hip (the per-step
// kernels of tg_kernels.h and tg_py1.h) and tg_flow.hip (k_flow, tg_flow.h).  __device__
// functions, types and constants only: no kernel and no host code, so an edit here changes both
// units and an edit anywhere else changes one.
//
// One wavefront lane per env.  Per launch every lane loads its env from struct-of-arrays
// HBM (16-B + 16-B + 8-B coalesced loads), runs the requested option to completion
// (_Option.run, OP/:20-36) over the level grid staged in LDS, writes obs / reward / valid /
// done, and stores the env back.  Auto-reset compacts completed episodes with a wavefront
// ballot + one atomic per wave.  No MFMA: the path is integer/branch work plus a handful of
// IEEE f64 ops (obs divisions, uniform/gauss), built with -ffp-contract=off.
//
// HBM layout per handle (N envs):
//   st4[N]  uint4   position, flags, object cells and MT state word (tg_core.h: the st4 codec)
//   ang[N]  double2 {handle0.angle, handle1.angle}
//   ep[N]   int2    {episode return, episode length}
//   mt[N][624] u32  env-major MT19937 words (2,496 B per env)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tg_amd.h"
#include "tg_core.h"
#include "tg_level.h"
#include "tg_batch.h"
#include "tg_twist.h"
#include "tg_run_diag.h"  // (k_run's timing hooks: no-ops outside the diagnostic build)

using namespace tg;

namespace {

constexpr int BLOCK = 256;
// k_run's workgroup: a workgroup holds its CU slot (LDS, wave slots) until its slowest wave
// ends, and k_run's waves differ in length by up to ~3x
#ifndef TG_RUN_BLOCK
#define TG_RUN_BLOCK 256
#endif
constexpr int RUN_BLOCK = TG_RUN_BLOCK;
static_assert(RUN_BLOCK % 64 == 0 && BLOCK % RUN_BLOCK == 0, "whole waves, whole k_classify blocks");
// issue priority of the option waves whose ticks are slow (ladders, drops, jumps), which share
// SIMDs with the go waves (0.153 vs 0.156 ms per step)
constexpr int PRIO_SLOW = 3;

// (the st4 words are packed and unpacked by tg_core.h's codec: pack, unpack, unpack_st4)

// The level in LDS: the bordered cell grid (per-lane indexed probes) and the trigger table
// (indexed per lane by the cascade; kernel arguments indexed per lane would be vector loads
// from the kernarg segment).
struct LdsLevel {
  uint32_t trig[12];
  uint32_t grid[MAX_CELLS / 4];
};
TG_HD int grid_words(int W, int H) { return ((W + 2 * PAD) * (H + 2 * PAD) + 3) / 4; }
// grid words, trigger table and (masks: non-null) the level bitmasks into LDS; NT: the
// workgroup's threads
template <int NT = BLOCK>
__device__ __forceinline__ void stage_cells(uint32_t* lgrid, uint32_t* ltrig,
                                            const uint32_t* __restrict__ grid, const Level& L,
                                            uint32_t* masks = nullptr) {
  const int nwords = grid_words(L.W, L.H);
  for (int i = threadIdx.x; i < nwords; i += NT) lgrid[i] = grid[i];
  if (threadIdx.x < 12) ltrig[threadIdx.x] = L.trig[threadIdx.x >> 1][threadIdx.x & 1];
  if (masks && L.masks)
    for (int i = threadIdx.x; i < mk_words(L.W, L.H); i += NT) masks[i] = L.masks[i];
  __syncthreads();
}
// what a kernel's lanes read of the staged level (win: the waves' areas, run_level_in_lds)
struct LevelView {
  const uint32_t* trig;
  Map m;
  uint8_t* win;
};
// the level staged in LDS of the calling kernel's own (includes the barrier)
__device__ __forceinline__ LevelView level_in_lds(const uint32_t* __restrict__ grid, const Level& L) {
  __shared__ LdsLevel lv;
  stage_cells(lv.grid, lv.trig, grid, L);
  return {lv.trig, Map{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H}, nullptr};
}
// k_run's and k_flow's LDS: the NT / 64 waves' areas (WAVE_BYTES each, the code windows, at offset
// 0: 16-B aligned for the LDS-DMA), then the level's grid words and bitmasks (Map::mk); includes
// the barrier.  (Sized at launch for the handle's level instead of the largest, with the rows'
// loads issued before the staging barrier, it measured ~4 % slower for the masked: DESIGN.md §3.1.)
// (run_lds_win: the waves' areas alone, nothing staged and no barrier: k_run's workgroups past
// every listed chunk, whose waves twist in theirs)
template <int NT, int WAVE_BYTES>
__device__ __forceinline__ uint8_t* run_lds_win() {
  __shared__ uint4 run_lds[((NT / 64) * WAVE_BYTES + MAX_CELLS + 4 * MK_MAX_WORDS) / 16];
  return reinterpret_cast<uint8_t*>(run_lds);
}
template <int NT, int WAVE_BYTES>
__device__ __forceinline__ LevelView run_level_in_lds(const uint32_t* __restrict__ grid, const Level& L) {
  __shared__ uint32_t ltrig[12];
  uint8_t* const win = run_lds_win<NT, WAVE_BYTES>();
  uint32_t* const lgrid = reinterpret_cast<uint32_t*>(win + (NT / 64) * WAVE_BYTES);
  uint32_t* const lmk = lgrid + grid_words(L.W, L.H);
  stage_cells<NT>(lgrid, ltrig, grid, L, lmk);
  return {ltrig, Map{reinterpret_cast<const uint8_t*>(lgrid), L.W, L.H, L.masks ? lmk : nullptr}, win};
}

__device__ __forceinline__ void store_obs(double* out, int64_t i, const double o[9]) {
  double* p = out + i * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) p[k] = o[k];
}

// ------------------------------------------------------------------------------------------
// CPython random for the option loops (k_run, k_step): tg::Rng's read-only consumption of the
// two pre-twisted generations, reading each draw's code byte (tg_core.h draw_code: its noisy /
// jump / flip outcomes) from a per-lane window in LDS.
//   Window: WIN_CHUNKS 16-B chunks (16 codes each) per lane, slot j of the wave's window at
//   m0 + j * 1 KB holding the lane's j-th chunk from where the window starts.  prime() fills
//   it with one LDS-DMA (global_load_lds_dwordx4) per slot: every lane's chunk j goes to slot
//   j, so M0 (which addresses the DMA's LDS destination and must be wave-uniform) is the same
//   for all of them and each slot costs ONE instruction.  The first draw waits for the DMAs
//   (s_waitcnt vmcnt(0), once per launch; k_run primes before the option's setup so the wait
//   is mostly covered); every later draw is an LDS byte read, issued one draw ahead.  The
//   window holds 112 draws, more than an option of the default level consumes in one step
//   (<= ~110); a lane that exhausts it refills it the same way (WAR: lgkmcnt(0) before the
//   DMAs; RAW: vmcnt(0) after) and pays one memory latency.  The DMAs are issued from inline
//   asm, invisible to the compiler's waitcnt pass, so no register copy of a loaded value is
//   waited for early (a register-held prefetch made the compiler wait at the load).
//   Position bookkeeping is deferred: the window start (pos) plus the draws taken since (n)
//   are folded into pos at a refill and at finish.
//   Stale halves: a window overlapping the half the lane is not in, while that half is stale
//   (crossed), is loaded only after the lane has regenerated that half itself (regen_half:
//   rare, > 312 draws since the refill; the refilling idle wave, if any, writes the same).
//   Draws that need the double (handle angles in a flip cascade, an auto-reset's uniform and
//   gauss) consume the code and read the position's two words (one 8-B load).
// ------------------------------------------------------------------------------------------
// code bytes per lane per LDS-DMA (global_load_lds_dwordx4).  The dword form (lane l's 4 B at
// M0 + 4l, no LDS bank conflicts) needs 4x the DMA instructions per fill and measured 7 %
// slower (profiles/r03/lds_window_ab.json)
constexpr int WIN_UNIT = 16;
constexpr int WIN_DRAWS = 64;                       // codes per lane in the window
constexpr int WIN_SLOTS = WIN_DRAWS / WIN_UNIT;     // DMA instructions per fill
constexpr int WIN_SLOT_BYTES = 64 * WIN_UNIT;       // one slot: every lane's unit
constexpr uint32_t CODE_UNITS = MT_CODES / WIN_UNIT;
static_assert(MT_CODES % WIN_UNIT == 0, "whole DMA units of codes per env");
constexpr int WIN_WAVE_BYTES = WIN_SLOTS * WIN_SLOT_BYTES;  // 4 KB per wave
constexpr int WAVE_SCRATCH = MT_N * 4;                       // wave_twist's scratch (aliases it)
static_assert(WIN_WAVE_BYTES >= WAVE_SCRATCH, "wave_refill reuses the window as scratch");
static_assert(WIN_DRAWS - WIN_UNIT + 1 >= (int)MAX_TICK_DRAWS, "a refilled window holds a tick's draws");

// LDS-DMA of one WIN_UNIT-byte unit per active lane into LDS [m0 + lane * WIN_UNIT]; M0 is
// saved/restored.  MOD: the load's cache modifiers ("": none)
#define TG_GLDS_UNIT(MOD, m0, gptr)                                       \
  do {                                                                    \
    uint32_t save_;                                                       \
    asm volatile(                                                         \
        "s_mov_b32 %0, m0\n\t"                                            \
        "s_mov_b32 m0, %1\n\t"                                            \
        "s_nop 0\n\t"                                                     \
        "global_load_lds_dwordx4 %2, off" MOD "\n\t"                      \
        "s_mov_b32 m0, %0"                                                \
        : "=&s"(save_)                                                    \
        : "s"(__builtin_amdgcn_readfirstlane(m0)), "v"(gptr)              \
        : "memory");                                                      \
  } while (0)

// the rare second crossing (RngCodes::fill), out of line so that the draw sites stay small, its
// generation loops out of line too: a callee's registers add to its caller's allocation (k_run
// 104 VGPRs, 4 waves per SIMD, with them inline)
__device__ __noinline__ void twist_gen_call(const uint32_t* src, uint32_t* dst) { twist_gen(src, dst); }
__device__ __noinline__ void gen_codes_call(const uint32_t* w, uint8_t* c) { gen_codes(w, c); }
struct GenCalls {
  __device__ void twist(const uint32_t* src, uint32_t* dst) const { twist_gen_call(src, dst); }
  __device__ void codes(const uint32_t* w, uint8_t* c) const { gen_codes_call(w, c); }
};
__device__ __noinline__ void regen_half(uint32_t* mt, uint8_t* mc, uint32_t h) {
  twist_half(mt, h, mc, false, GenCalls());
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
}

// How a kernel reaches the env state and the MT ring in HBM: the memory model that load_env,
// store_env, RngCodesT and the step's epilogue (finish_env, run_epilogue, run_listed) are written
// over.  This is the per-step kernels' model: whoever wrote those bytes was an earlier launch on
// the stream or this lane itself, so stream order makes them visible and plain loads, plain stores
// and the plain LDS-DMA do; the one wait is the window's, landed before the first result store.
// (k_flow hands envs from wave to wave inside one launch: its model is tg_flow.h's, beside the
// coherence rules it implements.)
struct LaunchMem {
  // one env's state words at index `at` of their arrays.  (Each word is copied whole before it is
  // assigned: the 16-B and 8-B vector loads.  Assigned straight from the array, or returned by
  // value from a function, the compiler splits them into dword loads and k_classify, k_step and
  // k_serve1 take 2-3 more VGPRs.)
  static __device__ __forceinline__ void load(const uint4* st4, const double2* ang, const int2* ep,
                                              int64_t at, uint4& s4, double2& a2, int2& e2) {
    const uint4 s = st4[at];
    s4 = s;
    const double2 a = ang[at];
    a2 = a;
    const int2 p = ep[at];
    e2 = p;
  }
  // ep_too false: the episode words are unchanged, a reward-None step: no store.  (ep by value,
  // as store_env takes it: profiles/headers/isa_compare.log)
  static __device__ __forceinline__ void store(const Soa& S, int64_t i, const Env& e, int2 ep,
                                               bool ep_too) {
    S.st4[i] = pack(e);
    S.ang[i] = make_double2(e.ang0, e.ang1);
    if (ep_too) S.ep[i] = ep;
  }
  // the code window's DMA, a stale half's per-lane regeneration, a draw's two words
  static __device__ __forceinline__ void glds(uint32_t m0, const void* gptr) { TG_GLDS_UNIT("", m0, gptr); }
  static __device__ __forceinline__ void regen(uint32_t* mt, uint8_t* mc, uint32_t h) { regen_half(mt, mc, h); }
  static __device__ __forceinline__ WordPair pair(const uint32_t* mt, uint32_t p) { return mt_pair_ool(mt, p); }
  // The step's epilogue lands the window before its first result store: stores count in vmcnt
  // too, so a wait placed after them is a wait for their acknowledgement.  Then nothing is in
  // flight at RngCodesT::finish, and no wait stands behind those stores; a caller that did not
  // (k_reset) still lands its window there.
  template <class R>
  static __device__ __forceinline__ void before_rows(R& rng) { rng.drain(); }
  template <class R>
  static __device__ __forceinline__ void at_finish(R& rng) { rng.drain(); }
};
// one env's state words: from the arrays st4 / ang / ep at index at (the handle's, or k_run's
// worklist-ordered copies), and back to the handle's.  Mem: the kernel's memory model
template <class Mem>
__device__ __forceinline__ void load_env(const uint4* st4, const double2* ang, const int2* ep, int64_t at,
                                         uint4& s4, double2& a2, int2& e2) {
  Mem::load(st4, ang, ep, at, s4, a2, e2);
}
template <class Mem>
__device__ __forceinline__ void load_env(const uint4* st4, const double2* ang, const int2* ep, int64_t at,
                                         Env& e, int2& e2) {
  uint4 s4;
  double2 a2;
  load_env<Mem>(st4, ang, ep, at, s4, a2, e2);
  unpack(s4, a2, e);
}
template <class Mem>
__device__ __forceinline__ void store_env(const Soa& S, int64_t i, const Env& e, int2 ep, bool ep_too = true) {
  Mem::store(S, i, e, ep, ep_too);
}

template <class Mem = LaunchMem>
struct RngCodesT {
  static constexpr uint32_t NONE = 0xFFFFFFFFu;
  uint32_t* mt;      // this env's MT_STORE stored words (HBM)
  uint8_t* mc;       // this env's MT_CODES code bytes (HBM)
  lds_u8* cell;      // this lane's unit in slot 0 of the wave's window
  uint32_t m0;       // LDS address of slot 0 of the wave's window (wave-uniform)
  uint32_t pos;      // word position of the window's first draw (even)
  uint32_t n;        // draws taken since then
  uint32_t rd;       // LDS offset of the next draw's code from cell: slot * 1 KB + byte
  uint32_t left;     // draws left in the window
  uint32_t nxc;      // the next draw's code (read one draw ahead)
  uint32_t stale;    // word offset (0 / 624) of the half that is two generations behind, or NONE
  uint32_t tag;      // the state word's MT_STALE | MT_LISTED bits on entry
  uint32_t draws;
  uint32_t regens;   // halves this lane regenerated itself (regen_half)
  bool primed, loaded, entered;  // entered: a half was entered in this launch (as tg::Rng)

  __device__ __forceinline__ RngCodesT(uint32_t* m, uint8_t* c, uint32_t state, lds_u8* wave_win)
      : mt(m), mc(c), cell(wave_win + (threadIdx.x & 63) * WIN_UNIT),
        m0(__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)wave_win)),
        pos(state & MT_POS_MASK), n(0u), rd(0u), left(0u), nxc(0u),
        stale((state & MT_STALE) ? (uint32_t)MT_HALF - mt_half(state & MT_POS_MASK) : NONE),
        tag(state & (MT_STALE | MT_LISTED)),
        draws(0u), regens(0u), primed(false), loaded(false), entered(false) {}

  // fold the draws taken since the window start into pos (a window is < MT_HALF / 2 draws, so
  // at most one half boundary lies in between).  Entering a half that is stale (possible only
  // when the window ended exactly at the boundary, so nothing of it was read) regenerates it
  // first, from the half being left, which then becomes the stale one.
  __device__ __forceinline__ void sync() {
    const uint32_t d = pos >> 1, e = d + n;
    if (e / (MT_HALF / 2) != d / (MT_HALF / 2)) {
      const uint32_t left_half = mt_half(pos), entered_half = (uint32_t)MT_HALF - left_half;
      if (stale == entered_half) {
        Mem::regen(mt, mc, entered_half);
        ++regens;
      }
      stale = left_half;
      entered = true;
    }
    pos = 2u * (e >= (uint32_t)MT_CODES ? e - (uint32_t)MT_CODES : e);
    n = 0u;
  }
  // DMA the window starting at pos (all lanes reaching it start at slot 0: one DMA per slot)
  __device__ __forceinline__ void fill() {
    const uint32_t d = pos >> 1, c0 = d / (uint32_t)WIN_UNIT;
    if (stale != NONE) {
      // the draws the window serves are words [pos, pos + 2 * left) (mod MT_WORDS; the bytes of
      // its first and last chunks outside that range are never read): regenerate the stale
      // half first if they overlap it
      const uint32_t w0 = pos, w1 = pos + 2u * ((uint32_t)WIN_DRAWS - d % (uint32_t)WIN_UNIT);
      if ((w0 < stale + (uint32_t)MT_HALF && stale < w1) ||
          (w1 > (uint32_t)MT_WORDS && stale < w1 - (uint32_t)MT_WORDS)) {
        Mem::regen(mt, mc, stale);
        ++regens;
        stale = NONE;
      }
    }
#pragma unroll
    for (int j = 0; j < WIN_SLOTS; ++j) {
      const uint32_t c = c0 + j < CODE_UNITS ? c0 + j : c0 + j - CODE_UNITS;
      Mem::glds(m0 + j * WIN_SLOT_BYTES, mc + c * (uint32_t)WIN_UNIT);
    }
    rd = d % (uint32_t)WIN_UNIT;
    left = (uint32_t)WIN_DRAWS - rd;
    loaded = false;
  }
  __device__ __forceinline__ uint32_t read() const {
    const uint32_t r = rd < (uint32_t)WIN_DRAWS ? rd : 0u;  // stay inside the window
    return cell[(r / WIN_UNIT) * WIN_SLOT_BYTES + r % WIN_UNIT];
  }
  __device__ __forceinline__ void prime() {
    fill();
    primed = true;
  }
  // at least k draws available in the window (the option loops call it once per tick: a tick
  // draws at most 6 times; an auto-reset 4); refilling is rare and has one site per loop
  __device__ __forceinline__ void reserve(uint32_t k) {
    if (!primed) prime();
    if (left < k) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // no read of the old window pending
      sync();
      fill();
    }
    land();
  }
  // the window's DMAs have landed (they are in flight only between a fill and this call); the
  // first draw's code is read ahead
  __device__ __forceinline__ void land() {
    if (!loaded) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      nxc = read();
      loaded = true;
    }
  }
  // at least k draws staged (no refill: the plain go loop's exit test)
  __device__ __forceinline__ bool has(uint32_t k) const { return left >= k; }
  // the code dword holding draws 4d .. 4d + 3 of the window (d < WIN_DRAWS / 4)
  __device__ __forceinline__ uint32_t dword(uint32_t d) const {
    return *reinterpret_cast<const lds_u32*>(cell + (4u * d / WIN_UNIT) * WIN_SLOT_BYTES +
                                             (4u * d) % WIN_UNIT);
  }
  // walk_ticks (tg_core.h) by multi-draw hops (walk_hops there: whole code dwords while all
  // four of their ticks are plain, the dword the walk ends in tick by tick), with walk_ticks's
  // result
  template <int DIR>
  __device__ __forceinline__ int walk(int& x, const int lim, const int cap) {
    const int taken = walk_hops<DIR>(*this, x, lim, cap);
    n += (uint32_t)taken;
    draws += (uint32_t)taken;
    nxc = read();  // code() reads one draw ahead
    return taken;
  }
  // the option loops' phase marks (tg_core.h counted_tick, span_loop): the diagnostic build's
  // per-phase clock, nothing in the product (tg_run_diag.h)
  RunPhaseClock clk;
  __device__ __forceinline__ void phase(int k) { clk.mark(k); }
  // a draw was taken past the staged window (reserve's bound broken: flagged E_WINDOW)
  __device__ __forceinline__ bool overrun() const { return left > (uint32_t)WIN_DRAWS; }
  // one draw, consumed for its outcomes (draw_code); reserve() guarantees it is in the window
  __device__ __forceinline__ uint32_t code() {
    const uint32_t c = nxc;
    ++n;
    ++draws;
    ++rd;
    --left;
    nxc = read();  // the next draw's code, one draw ahead (a byte of the window when left = 0)
    return c;
  }
  // one draw as its double (rare): the code is consumed too, the value built from the words
  // (an odd generation's twisted from the stored one before it, tg_core.h mt_pair)
  __device__ __forceinline__ double random() {
    uint32_t p = (pos >> 1) + n;
    p = 2u * (p >= (uint32_t)MT_CODES ? p - (uint32_t)MT_CODES : p);
    (void)code();
    const WordPair w = Mem::pair(mt, p);
    return mt_double(w.w0, w.w1);
  }
  __device__ __forceinline__ double uniform(double a, double b) { return a + (b - a) * random(); }
  // the window's DMAs have landed (the step's epilogue calls it before its first result store:
  // stores count in vmcnt too, so a wait placed after them is a wait for their acknowledgement)
  __device__ __forceinline__ void drain() {
    if (primed) land();
  }
  // drain the DMAs (the window is reused as scratch); returns the state word to store: the
  // entry's stale half, still stale, keeps its bits (listed or not); a half left in this launch
  // is stale and not listed yet; none, if the lane regenerated the stale half itself.
  // (Mem::at_finish: the model's wait for the window)
  __device__ __forceinline__ uint32_t finish() {
    Mem::at_finish(*this);
    sync();
    primed = loaded = false;
    return pos | (stale == NONE ? 0u : entered ? MT_STALE : tag);
  }
};

using RngCodes = RngCodesT<>;

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}
// For every lane in `need`: regenerate the stale half of its env (the one not holding the
// position in its state word), one env at a time, with the whole wave (wave_twist_gens: its
// MT_HALF_GENS generations from the other half's last).  Must be reached by all 64 lanes.
__device__ __forceinline__ void wave_refill(unsigned long long need, uint32_t* env_mt, uint8_t* env_mc,
                                            uint32_t state, lds_u32* scratch) {
  const uint32_t pos = state & MT_POS_MASK;
  const uint32_t dst = (uint32_t)MT_HALF - mt_half(pos);
  const uint64_t src_l = (uint64_t)(uintptr_t)(env_mt + regen_src_off(dst));
  const uint64_t w_l = (uint64_t)(uintptr_t)env_mt;
  const uint64_t c_l = (uint64_t)(uintptr_t)env_mc;
  const int g0_l = (int)(dst / (uint32_t)MT_N);
  while (need) {
    const int L = __ffsll((long long)need) - 1;
    need &= need - 1;
    wave_twist_gens((const glb_u32*)(uintptr_t)readlane64(src_l, L),
                    (glb_u32*)(uintptr_t)readlane64(w_l, L), (uint8_t*)(uintptr_t)readlane64(c_l, L),
                    __builtin_amdgcn_readlane(g0_l, L), MT_HALF_GENS, true, scratch);
  }
}

// 64-lane sum (wave64)
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

enum { ST_STEPS, ST_VALID, ST_TICKS, ST_DRAWS, ST_EPISODES, ST_EP_OVERFLOW, ST_REGENS, ST_WTICKS,
       ST_RQUIET,  // of ST_REGENS, the halves of k_run's quiet drain
       ST_TRUNC,   // of ST_EPISODES, those a step limit ended (k_timelimit, tg_timelimit.h)
       ST_COUNT };

// 64-lane max (wave64)
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// In-kernel span stamps of the timed launches (tg_set_timing): each wave's lane 0 folds its
// start and end (s_memrealtime: the 100 MHz constant clock) into one of KST_SLOTS
// (min start, max end) pairs of the launch's record, with returnless atomics on 64 addresses;
// flush_timing reduces them to the launch's span, first wave start to last wave end.  Null
// record: not timed (a wave-uniform branch).
constexpr int KST_SLOTS = 64;
constexpr int KST_STRIDE = 16;  // u64 per slot: each slot's pair in a 128-B line of its own
__device__ __forceinline__ unsigned long long kst_begin(const unsigned long long* ks) {
  return ks ? __builtin_amdgcn_s_memrealtime() : 0ull;
}
__device__ __forceinline__ void kst_end(unsigned long long* ks, unsigned long long t0) {
  if (ks && (threadIdx.x & 63) == 0) {
    unsigned long long* const s = ks + KST_STRIDE * (blockIdx.x % KST_SLOTS);
    atomicMin(s, t0);
    atomicMax(s + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}
struct StepIO {
  int32_t* __restrict__ actions;   // input; with policy >= 0 the step's actions are written here
  double* __restrict__ obs;
  int32_t* __restrict__ reward;
  uint8_t* __restrict__ valid;
  uint8_t* __restrict__ done;
  double* __restrict__ final_obs;  // may be null
  int policy;                      // -1: actions given; else TG_POLICY_* evaluated in the step
                                   // (selects the kernels' POL instantiation)
  uint64_t a0;                     // the policy's action seed and step index
  int64_t t;
  uint32_t tstep;                  // this step's index in the handle's step count (launch_step):
                                   // an episode's length is tstep + 1 - its start step (S.ep.y)
};

// (the synthetic policies' action, POL >= 0: tg_rules.h policy_action)
struct EpQueue {
  tg_episode* __restrict__ eps;
  int32_t* count;
  int32_t cap;
};

// Completed episodes (auto-reset): wavefront ballot, popcount prefix, one atomic per wave.
// The queue is drained by tg_episodes; if nobody drains it, the count must not run away (an
// int32 that wraps would turn the bound check into an out-of-bounds store): a wave whose
// records do not all fit clamps the count back to cap (atomicMin) after its add.  Between an
// add and its clamp other waves can add, so the count stays below cap + the records of the
// waves in flight (<= cap + n < 2^31 with cap <= 2^28 and n < 2^30); slots are compared
// unsigned.  The records that do not fit are counted per wave in the wave's own block slot.
// Must be reached by every lane of the wave.
__device__ __forceinline__ void record_episodes(bool mine, int64_t g, int2& ep, uint32_t tstep,
                                                const EpQueue& q, unsigned long long* stats,
                                                int64_t sl) {  // sl: the wave's stats slot
  const unsigned long long b = __ballot(mine);
  if (!b) return;
  const int lane = threadIdx.x & 63;
  const int first = __ffsll((long long)b) - 1;
  const int cnt = __popcll(b);
  int base = 0;
  if (lane == first) {
    base = atomicAdd(q.count, cnt);
    if ((uint32_t)base + (uint32_t)cnt > (uint32_t)q.cap) {
      atomicMin(q.count, q.cap);
      const uint32_t lost = (uint32_t)base >= (uint32_t)q.cap
                                ? (uint32_t)cnt : (uint32_t)base + (uint32_t)cnt - (uint32_t)q.cap;
      atomicAdd(&stats[(size_t)sl * ST_COUNT + ST_EP_OVERFLOW], (unsigned long long)lost);
    }
  }
  base = __shfl(base, first, 64);
  if (mine) {
    const uint32_t slot = (uint32_t)base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (slot < (uint32_t)q.cap) {
      tg_episode r;
      r.env = g;
      r.ret = ep.x;
      r.len = (int32_t)(tstep + 1u - (uint32_t)ep.y);
      q.eps[slot] = r;
    }
    ep = make_int2(0, (int32_t)(tstep + 1u));  // the next episode starts with the next step
  }
}

// Launch counters: every step kernel has a per-block slot of `part` ([grid][ST_COUNT]) and the
// host sums the slots on demand (one counter word per launch took ~32k same-line atomics:
// ~370 us at ~88 atomics/us).  Each wave's lane 0 adds its sums into its block's slot with
// returnless atomics (no contention across blocks; no barrier, so every wave exits as soon as
// it is done).  Must be reached by every lane of the wave.
// wave_ticks: the wave's longest lane's ticks (the tick loop's trip count, lane efficiency).
__device__ __forceinline__ void wave_stats(unsigned long long* __restrict__ part, int steps,
                                           int valid, int ticks, int draws, int episodes,
                                           int regens = 0, bool wave_ticks = false,
                                           int64_t sl = -1) {  // slot: blockIdx.x by default
  // a counter that is 0 on every lane (k_run's steps / valid, most waves' episodes) skips its
  // six cross-lane steps: the reductions sit in the option waves' epilogue, on the tail
  auto sum = [](int x) { return __ballot(x != 0) ? wave_sum(x) : 0; };
  const int v[5] = {sum(steps), sum(valid), sum(ticks), sum(draws), sum(episodes)};
  const int wt = wave_ticks ? wave_max(ticks) : 0;
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* const slot = part + (size_t)(sl < 0 ? (int64_t)blockIdx.x : sl) * ST_COUNT;
#pragma unroll
    for (int c = 0; c < 5; ++c)
      if (v[c]) atomicAdd(&slot[c], (unsigned long long)v[c]);
    if (regens) atomicAdd(&slot[ST_REGENS], (unsigned long long)regens);
    if (wt) atomicAdd(&slot[ST_WTICKS], (unsigned long long)wt);
  }
}

// wave_stats for a wave whose only live lane is lane 0 (k_py1, k_serve1): lane 0's own values,
// no cross-lane reductions (~0.5 us of a one-env call)
__device__ __forceinline__ void lane0_stats(unsigned long long* __restrict__ part, int steps,
                                            int valid, int ticks, int draws, int episodes,
                                            int regens = 0, bool wave_ticks = false) {
  if ((threadIdx.x & 63) != 0) return;
  unsigned long long* const slot = part + (size_t)blockIdx.x * ST_COUNT;
  const int v[5] = {steps, valid, ticks, draws, episodes};
#pragma unroll
  for (int c = 0; c < 5; ++c)
    if (v[c]) atomicAdd(&slot[c], (unsigned long long)v[c]);
  if (regens) atomicAdd(&slot[ST_REGENS], (unsigned long long)regens);
  if (wave_ticks && ticks) atomicAdd(&slot[ST_WTICKS], (unsigned long long)ticks);
}

// finish one env-step: obs/reward/valid/done rows, episode counters, optional auto-reset.
// keep != nullptr: the obs row is returned there instead of stored (the caller stores it).
// The option waves' epilogue computes its obs rows by f64 division: the quotient table
// (tg_core.h obs_div) is a global load on their tail, and by stamps the epilogue was ~4,000
// cycles shorter without it (profiles/r04/stamps_divq_uniform_r04k.log); k_classify, whose
// waves are not a tail, keeps the table
__device__ __forceinline__ Level level_div(const Level& L) {
  Level d = L;
  d.obs_q = nullptr;
  return d;
}
// VALID: the valid row is this call's (k_classify writes every env's valid row itself, coalesced:
// k_run's scattered byte store cost a 32-B write granule per listed env)
template <bool AUTORESET, bool FINAL, bool VALID = true, class R>
__device__ __forceinline__ void finish_step(const Level& L, Env& e, R& rng, int64_t i,
                                            const StepResult& r, int2& ep, const StepIO& io,
                                            double* keep = nullptr) {
  if (rng.overrun()) e.f |= E_WINDOW;
  double o[9];
  observe(L, e, o);  // get_state (TG/:94)
  io.reward[i] = r.reward;
  if (VALID) io.valid[i] = (uint8_t)r.ran;
  io.done[i] = (uint8_t)r.done;
  ep.x += r.reward;  // (ep.y, the episode's start step, stays: no store for a reward-None step)
  if (FINAL) store_obs(io.final_obs, i, o);
  if (AUTORESET && r.done) {
    reset_env(L, e, rng);
    observe(L, e, o);
  }
  if (keep) {
#pragma unroll
    for (int k = 0; k < 9; ++k) keep[k] = o[k];
  } else {
    store_obs(io.obs, i, o);
  }
}

// The obs rows of a wave's 64 consecutive envs (4,608 B) through LDS: lane l stores the
// 8-B words l, l+64, ... of the span, so each store instruction writes 512 contiguous bytes
// (a lane storing its own 72-B row touches ~36 cache lines per instruction).  Rows of envs
// not in `mask` are left alone.  Every lane of the wave must reach it.
__device__ __forceinline__ void store_obs_wave(double* __restrict__ out, int64_t wave_first,
                                               unsigned long long mask, const double o[9],
                                               double* __restrict__ stage) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 9; ++k) stage[lane * 9 + k] = o[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double* const dst = out + wave_first * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int w = j * 64 + lane;
    if ((mask >> (w / 9)) & 1ull) __builtin_nontemporal_store(stage[w], dst + w);
  }
}

// ---- one env's step after its option (step_env; k_run's and k_flow's run_listed) ---------------
// The env's rows, its MT state word (a half left here: MT_STALE, listed by the next
// classification), the lane's draws and own regenerations, its error bits.  (Mem::before_rows:
// the model's wait for the window, if it takes it ahead of the result stores)
template <bool AUTORESET, bool FINAL, bool VALID, class Mem>
__device__ __forceinline__ void finish_env(const Level& L, Env& e, RngCodesT<Mem>& rng, int64_t i,
                                           const StepResult& r, int2& ep, const StepIO& io,
                                           uint32_t* err_or, uint32_t& draws, int& lregen) {
  Mem::before_rows(rng);
  finish_step<AUTORESET, FINAL, VALID>(level_div(L), e, rng, i, r, ep, io);
  e.mti = rng.finish();
  draws = rng.draws;
  lregen = (int)rng.regens;
  if (e.f & E_MASK) atomicOr(err_or, e.f & E_MASK);
}
// The wave's epilogue: completed episodes, the envs' state back, the launch counters (slot sl).
// ep_in: the episode words as loaded (stored only if changed), or null (always stored).  steps /
// valid / wregens: counted where the caller steps whole envs.  Every lane of the wave reaches it.
template <bool AUTORESET, class Mem, bool ONE = false>  // ONE: only lane 0 live (k_serve1)
__device__ __forceinline__ void run_epilogue(const Soa& S, bool live, int64_t i, int64_t g, const Env& e,
                                             int2& ep, const int2* ep_in, const StepResult& r,
                                             uint32_t draws, int lregen, uint32_t tstep, const EpQueue& q,
                                             unsigned long long* __restrict__ stats, int64_t sl, int steps = 0,
                                             int valid = 0, int wregens = 0) {
  if (AUTORESET) record_episodes(live && r.done, g, ep, tstep, q, stats, sl);
  if (live) store_env<Mem>(S, i, e, ep, !ep_in || ep.x != ep_in->x || ep.y != ep_in->y);
  __builtin_amdgcn_s_setprio(0);
  const int eps = AUTORESET ? (live && r.done) : 0;
  if constexpr (ONE)
    lane0_stats(stats, steps, valid, r.ticks, (int)draws, eps, wregens + lregen, true);
  else
    wave_stats(stats, steps, valid, r.ticks, (int)draws, eps,
               wregens + (__ballot(lregen != 0) ? wave_sum(lregen) : 0), true, sl);
}
// ---- one-pass step: one lane per env, the option runs in place (TG_MODE_DIRECT) ----------
constexpr int POL_IMMEDIATE = -2;  // k_step's action is io.a0 (tg_step1), not an array entry
// POL: -1 actions given; POL_IMMEDIATE one action for all (tg_step1); else the TG_POLICY_*
// evaluated here (tg_rollout).  A template
// parameter, so the per-step kernels carry none of the policy's code or registers.
// One step of env i (lane i's; live iff i < n) with the level in LDS (trig, m) and the wave's
// code window wscr: k_step's body, also k_serve1's private-stream step.  Every lane of the wave
// must reach it.
template <bool AUTORESET, bool FINAL, int POL, bool ONE = false>  // ONE: only lane 0 live (k_serve1)
__device__ __forceinline__ StepResult step_env(const Soa& S, int64_t n, const Level& L,
                                         const uint32_t* trig, const Map& m, lds_u8* wscr,
                                         int64_t i, const StepIO& io, const EpQueue& q,
                                         int64_t g0, unsigned long long* __restrict__ stats,
                                         uint32_t* __restrict__ err_or) {
  const bool live = i < n;
  StepResult r{0, 0, 0, 0};
  uint32_t draws = 0;
  int lregen = 0;  // halves this lane regenerated in its option loop
  Env e;
  e.mti = 0u;
  int2 ep = make_int2(0, 0), ep_in = ep;
  if (live) {
    load_env<LaunchMem>(S.st4, S.ang, S.ep, i, e, ep);
    ep_in = ep;
    RngCodes rng(S.mt + i * MT_STORE, S.mc + i * MT_CODES, e.mti, wscr);
    int act;
    if constexpr (POL >= 0) {
      act = policy_action(L, m, e, POL, io.a0, g0 + i, io.t);
      if (io.actions) io.actions[i] = act;
    } else if constexpr (POL == POL_IMMEDIATE) {
      act = (int)(int64_t)io.a0;  // tg_step1: the action is a kernel argument
    } else {
      act = io.actions[i];
    }
    r = env_step(L, trig, m, e, act, rng);
    finish_env<AUTORESET, FINAL, true>(L, e, rng, i, r, ep, io, err_or, draws, lregen);
  }
  // one pass, no classify pass after it: regenerate the halves left in this launch now
  const unsigned long long need = __ballot(live && (e.mti & MT_STALE));
  wave_refill(need, S.mt + (live ? i : 0) * MT_STORE, S.mc + (live ? i : 0) * MT_CODES, e.mti,
              (lds_u32*)wscr);
  e.mti &= ~(MT_STALE | MT_LISTED);
  run_epilogue<AUTORESET, LaunchMem, ONE>(S, live, i, g0 + i, e, ep, &ep_in, r, draws, lregen, io.tstep, q,
                                      stats, blockIdx.x, live ? 1 : 0, r.ran, __popcll(need));
  return r;
}

// ---- the compacted step's lists (k_classify / k_run, tg_kernels.h; k_flow's chunks, tg_flow.h) --
constexpr int SHARDS = 8;  // the stale-MT-half refill lists: one per XCD (k_regen's waves of XCD x drain list x)
// the worklists' shards (k_classify's workgroup b appends to shard b % WSHARDS): each
// (option, shard) counter takes one returning atomic per workgroup that lists an env of that
// option, so more shards spread a launch's ~4k x 10 atomics over more words
#ifndef TG_WSHARDS
#define TG_WSHARDS 8
#endif
constexpr int WSHARDS = TG_WSHARDS;
// Worklists: one per option, and one (L_RESET) of the envs whose option cannot run but which
// enter the step done with auto-reset on (stepped with auto-reset off until done, then on):
// k_run resets them (reward None, no option), so k_classify carries no reset path (the gauss
// pair's f64 library code held it at 79 VGPRs, 6 waves per SIMD; without it 58, 8 waves)
constexpr int L_RESET = O_COUNT;
constexpr int NLIST = O_COUNT + 1;
// the run order of the lists (k_run, tg_kernels.h: why this order), and its inverse
struct RunOrder {
  int list[NLIST];      // the list run at position j
  int seg_base[NLIST];  // list k's first segment: its run position * WSHARDS
};
constexpr RunOrder make_run_order() {
  RunOrder r{{O_JUMP_LEFT, O_JUMP_RIGHT, O_GO_LEFT, O_GO_RIGHT, O_DOWN_LEFT, O_DOWN_RIGHT,
              O_UP_LADDER, O_DOWN_LADDER, O_INTERACT, L_RESET},
             {}};
  for (int j = 0; j < NLIST; ++j) r.seg_base[r.list[j]] = j * WSHARDS;
  return r;
}
constexpr RunOrder kRunOrder = make_run_order();
constexpr int NSEG = NLIST * WSHARDS;  // segment = run position * WSHARDS + shard
static_assert(NSEG <= 2 * RUN_BLOCK, "k_run's prefix: two segments per thread");
// the step's counters: the worklists', then the quiet lists' lengths (one per shard)
constexpr int QCTR = NSEG;
constexpr int NCTR = NSEG + SHARDS;
constexpr int CTR_STRIDE = 32;  // counters 128 B apart
// k_run's grid covers the envs rounded up to a k_classify workgroup plus RUN_EXTRA lanes, and
// its chunk space ends at or before listed + NLIST * 63 (each list padded to whole chunks) <=
// n + NLIST * 63 < the grid's lanes; both are whole waves, so at least one wave of every k_run
// grid has no chunk, at every batch size: the quiet lists are always drained (k_run)
constexpr int RUN_EXTRA = NLIST * 64;
static_assert(RUN_EXTRA > NLIST * 63 && BLOCK % 64 == 0 && RUN_BLOCK % 64 == 0,
              "a k_run grid always has a wave without a chunk");
struct Work {
  int32_t* __restrict__ lists;   // [NSEG][shard_cap], segment = run position * WSHARDS + shard
  // the listed envs' state, in worklist order (written by k_classify, which has loaded it
  // anyway): k_run reads its chunk's 64 records coalesced, in one round trip with the list
  // entries, instead of a dependent gather of 16 + 16 + 8 scattered bytes per lane
  uint4* __restrict__ wst4;      // [NSEG][shard_cap]
  double2* __restrict__ wang;
  int2* __restrict__ wep;
  int32_t* __restrict__ ctr;     // [NCTR * CTR_STRIDE], this step's counters
  int32_t* __restrict__ ctr_next;  // the other parity's, zeroed here for the next step
  // stale MT halves, one list per shard (= blockIdx.x % SHARDS, the XCD), appended across the
  // pending steps: list x at refill[x * rcap ..], its length at rcnt[x * CTR_STRIDE]
  uint32_t* __restrict__ refill;  // env | source half
  int32_t* __restrict__ rcnt;
  int64_t rcap;
  int64_t shard_cap;
  // the stale halves of this step's quiet envs (live, in no worklist: nothing but k_run's quiet
  // drain touches them before the next k_classify), one list per shard, one step's entries:
  // list x at quiet[x * qcap ..], its length at ctr[(QCTR + x) * CTR_STRIDE]
  uint32_t* __restrict__ quiet;
  int64_t qcap;
};
// k_regen (tg_kernels.h) drains the stale-MT-half refill lists every REGEN_STEPS compact steps
constexpr int REGEN_STEPS = 16;
// regen_ctr, per set: the 8 grab counters, then the 8 list lengths (k_classify's rcnt)
constexpr int RCTR_LIST = 8;
constexpr int RCTR_N = 16;

// ---- one env's step in two halves: decide (k_classify, k_flow's classification) and run (k_run,
// k_flow's run items) ------------------------------------------------------------------------------
struct EnvClass {
  bool runs, rst;  // the option can run; it cannot, and the env enters done with auto-reset on
  bool stale;      // its stale MT half goes on the refill list now
  int bk;          // the env's worklist (rst: L_RESET), -1: none (its step is none_rows')
};
// POL >= 0: the rollout's on-device policy (tg_rollout), its action written to io.actions (if
// given); else act_in.  Sets E_ACTION; marks a half left stale and not listed yet MT_LISTED:
// k_regen regenerates the lists of several steps at once (a lane that needs a half first does it
// itself: the ring leaves >= ~2,400 draws of slack, launch_step)
template <bool AUTORESET, int POL>
__device__ __forceinline__ EnvClass classify_env(const Level& L, const Map& m, Env& e, bool live,
                                                 int act, const StepIO& io, int64_t i, int64_t g) {
  EnvClass c{false, false, false, -1};
  int k = -1;
  if (live) {
    if constexpr (POL >= 0) {
      act = policy_action(L, m, e, POL, io.a0, g, io.t);
      if (io.actions) io.actions[i] = act;
    }
    k = option_index(act);
    c.runs = k >= 0 && can_run(L, m, e, k);
    if (k < 0) e.f |= E_ACTION;
  }
  c.rst = AUTORESET && live && !c.runs && is_done(e);
  c.bk = c.runs ? k : c.rst ? L_RESET : -1;
  c.stale = live && (e.mti & (MT_STALE | MT_LISTED)) == MT_STALE;
  if (c.stale) e.mti |= MT_LISTED;
  return c;
}
// a refill list's entry: env | source half
__device__ __forceinline__ uint32_t refill_entry(int64_t i, uint32_t mti) {
  return (uint32_t)i | (mt_half(mti & MT_POS_MASK) ? 0x80000000u : 0u);
}
// Up to 64 refill entries, one per lane (mine: this lane holds one, of env env_l), claimed and
// regenerated by the whole wave: k_regen's and k_run's quiet drain's body.  The claim clears
// MT_STALE | MT_LISTED in the env's state word by an atomic AND, and the half is regenerated only
// if that clear found MT_STALE: the half not holding the position, from the last generation of
// the one holding it.  An env can be listed twice before a drain (its lane regenerated the listed
// half itself, crossed again, and the next k_classify listed the new stale half): both entries
// name the half not holding the position, and the second claim finds it clean (round 4
// regenerated such a half once per entry: 20,320 vs 15,360 halves on the corridor level).
// Entries of one call for one env are serialised at the word's L2 channel.  Returns the halves
// regenerated; scr: the wave's WAVE_SCRATCH bytes of LDS.  Every lane of the wave reaches it.
template <bool NT>
__device__ __forceinline__ int regen_entries(const Soa& S, bool mine, uint32_t env_l, lds_u32* scr) {
  uint32_t* const st_w = reinterpret_cast<uint32_t*>(S.st4);  // word 4i + 3: env i's MT word
  const uint32_t st_l = mine ? atomicAnd(&st_w[(int64_t)env_l * 4 + 3], ~(MT_STALE | MT_LISTED)) : 0u;
  unsigned long long need = __ballot(mine && (st_l & MT_STALE));
  int halves = 0;
  // one half at a time: 52 VGPRs in k_regen, 8 waves per SIMD (the next half's source loads
  // pipelined into this one's twist took 76 VGPRs, 6 waves, and measured no faster: DESIGN.md §3.3)
  while (need) {
    const int L = __ffsll((long long)need) - 1;
    need &= need - 1;
    const uint32_t env = __builtin_amdgcn_readlane(env_l, L), s = __builtin_amdgcn_readlane(st_l, L);
    const uint32_t dst = (uint32_t)MT_HALF - mt_half(s & MT_POS_MASK);
    uint32_t* const mt = S.mt + (int64_t)env * MT_STORE;
    TwistIn t;
    twist_load((const glb_u32*)(mt + regen_src_off(dst)), t);
    twist_chain<NT>(t, (glb_u32*)mt, S.mc + (int64_t)env * MT_CODES, (int)(dst / (uint32_t)MT_N),
                    MT_HALF_GENS, true, scr);
    ++halves;
  }
  return halves;
}
// the step of the wave's envs whose option cannot run (fin; not L_RESET's): reward None, state
// unchanged (TG/:91-96, OP/:22-23), the obs rows through the wave's LDS `stage`.  The valid row
// is the caller's.  Every lane of the wave reaches it.
template <bool FINAL>
__device__ __forceinline__ void none_rows(const Level& L, const Soa& S, bool fin, Env& e, double2 a2,
                                          int64_t i, int2& ep, const StepIO& io, double* stage,
                                          uint32_t* err_or) {
  double orow[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (fin) {
    e.ang0 = a2.x;
    e.ang1 = a2.y;
    Rng rng(S.mt + i * MT_STORE, e.mti, S.mc + i * MT_CODES);  // no draws without a reset
    StepResult r{0, 0, (int)is_done(e), 0};
    finish_step<false, FINAL, false>(L, e, rng, i, r, ep, io, orow);
    if (e.f & E_MASK) atomicOr(err_or, e.f & E_MASK);
  }
  store_obs_wave(io.obs, i - (threadIdx.x & 63), __ballot(fin), orow, stage);
}
// the wave's lanes grouped by list (bk >= 0): the lane's rank in its group, the group's first
// lane and its size.  Must be reached by every lane of the wave.
struct LaneGroup {
  int rank, lead, nb;
};
__device__ __forceinline__ LaneGroup lane_groups(int bk) {
  LaneGroup g{0, 0, 0};
  unsigned long long pend = __ballot(bk >= 0);
  while (pend) {
    const int first = __ffsll((long long)pend) - 1;
    const int b0 = __builtin_amdgcn_readlane(bk, first);
    const unsigned long long b = __ballot(bk == b0);
    if (bk == b0) g = {(int)__popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull)), first, (int)__popcll(b)};
    pend &= ~b;
  }
  return g;
}
// A listed env's step from its loaded state through its rows (valid: the deciding pass's): option
// k, wave-uniform (one specialised loop; L_RESET: none, reward None).  hook: RunStamp or NoRunHook
template <bool AUTORESET, bool FINAL, class Mem, class Hook>
__device__ __forceinline__ void run_listed(const Level& L, const uint32_t* trig, const Map& m, const Soa& S,
                                           int64_t i, int k, Env& e, int2& ep, lds_u8* wscr,
                                           const StepIO& io, uint32_t* err_or, StepResult& r,
                                           uint32_t& draws, int& lregen, Hook& hook) {
  RngCodesT<Mem> rng(S.mt + i * MT_STORE, S.mc + i * MT_CODES, e.mti, wscr);
  rng.prime();  // issue the code loads now; the first draw comes after the policy setup
  hook.env_loaded();
  if (k != O_GO_LEFT && k != O_GO_RIGHT && k != O_INTERACT) __builtin_amdgcn_s_setprio(PRIO_SLOW);
  if (k != L_RESET) run_option(L, trig, m, e, k, rng, r);
  hook.option_done(rng.clk);
  r.done = is_done(e);
  finish_env<AUTORESET, FINAL, false>(L, e, rng, i, r, ep, io, err_or, draws, lregen);
}
}  // namespace

// k_flow<AR, POL> is instantiated in its own translation unit, tg_flow.hip, which is built
// without MachineLICM (the pass hoisted values out of the flow's work loop and
// held them live across it, 123-182 VGPRs; without it 121-129, 4 waves per SIMD)
namespace tg {
const void* flow_kernel(bool ar, int pol);
}
