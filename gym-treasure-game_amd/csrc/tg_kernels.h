// tg_kernels.h — the batch kernels: creation and reset, the one-pass and the two-pass step,
// k_regen, the flow mode's census and check, and the small per-env queries.  Compiled by
// tg_amd.hip only, whose host code launches them.  One env's step is tg_dev.h's, shared with k_flow:
// step_env (k_step); classify_env, none_rows, lane_groups (k_classify); run_listed, run_epilogue (k_run).
#pragma once
#include "tg_dev.h"
#include "tg_flow.h"
#include "tg_policy_mlp.h"
#include "tg_snapshot.h"

namespace {

// every in-kernel span record to (no start, no end) (kst_begin / kst_end, tg_dev.h)
__global__ void k_kst_init(unsigned long long* ks, int64_t slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < slots) {
    ks[KST_STRIDE * i] = ~0ull;
    ks[KST_STRIDE * i + 1] = 0ull;
  }
}

// ---- creation and reset ---------------------------------------------------------------------
// random.seed(seed0 + i): init_by_array into half 0's last stored slot (tg_core.h init_mt);
// k_gen_twist then makes the ring's 2 x MT_HALF_GENS generations from it, and k_reset (mask NULL)
// performs the constructor's game build (_TreasureGameImpl.__init__, IM/:31-53: 4 draws) —
// tg_create.
__global__ __launch_bounds__(BLOCK) void k_create(Soa S, int64_t n, uint64_t seed0,
                                                   const uint32_t* __restrict__ genrand) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  seed_mt(S.mt + i * MT_STORE + MT_SEED_OFF, genrand, seed0 + (uint64_t)i);
  Env e{};
  e.mti = 0u;
  S.st4[i] = pack(e);
  S.ang[i] = make_double2(0.0, 0.0);
  S.ep[i] = make_int2(0, 0);
}
// `gens` generations for every env, in sequence after the stored words at offset src: ring
// generations g0, g0 + 1, ... (codes; words of the even ones; tg_create, tg_write_state)
__global__ __launch_bounds__(BLOCK) void k_gen_twist(Soa S, int64_t n, uint32_t src, int g0,
                                                     int gens) {
  __shared__ __attribute__((aligned(16))) uint32_t scratch[BLOCK / 64][MT_N];
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  unsigned long long need = __ballot(i < n);
  const int64_t i0 = i - (threadIdx.x & 63);
  while (need) {
    const int L = __ffsll((long long)need) - 1;
    need &= need - 1;
    const int64_t e = i0 + L;
    wave_twist_gens((const glb_u32*)(S.mt + e * MT_STORE + src), (glb_u32*)(S.mt + e * MT_STORE),
                    S.mc + e * MT_CODES, g0, gens, false, (lds_u32*)scratch[threadIdx.x >> 6]);
  }
}

// the draw codes of the ring's first generation (stored words [0, 624)) of every env (tg_write_state)
__global__ __launch_bounds__(BLOCK) void k_gen_codes(Soa S, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) gen_codes(S.mt + i * MT_STORE, S.mc + i * MT_CODES);
}

__global__ __launch_bounds__(BLOCK) void k_reset(Soa S, int64_t n, Level L,
                                                  const uint8_t* __restrict__ mask,
                                                  double* __restrict__ obs, uint32_t tstep) {
  __shared__ __attribute__((aligned(16))) uint32_t scratch[BLOCK / 64][MT_N];
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  const bool reset = live && (!mask || mask[i]);
  Env e;
  e.mti = 0u;
  if (live) {
    unpack(S.st4[i], S.ang[i], e);
    if (reset) {
      Rng rng(S.mt + i * MT_STORE, e.mti, S.mc + i * MT_CODES);
      reset_env(L, e, rng);
      e.mti = rng.finish();
    }
    if (obs) {
      double o[9];
      observe(L, e, o);
      store_obs(obs, i, o);
    }
  }
  const bool stale = reset && (e.mti & MT_STALE);
  wave_refill(__ballot(stale), S.mt + (live ? i : 0) * MT_STORE, S.mc + (live ? i : 0) * MT_CODES, e.mti,
              (lds_u32*)scratch[threadIdx.x >> 6]);
  if (reset) {
    e.mti &= ~(MT_STALE | MT_LISTED);
    S.st4[i] = pack(e);
    S.ang[i] = make_double2(e.ang0, e.ang1);
    S.ep[i] = make_int2(0, (int32_t)tstep);  // the episode starts with the next step
  }
}

// ---- one-pass step (TG_MODE_DIRECT): step_env (tg_dev.h) per lane -------------------------
template <bool AUTORESET, bool FINAL, int POL = -1>
__global__ __launch_bounds__(BLOCK) void k_step(Soa S, int64_t n, Level L,
                                                 const uint32_t* __restrict__ grid, StepIO io,
                                                 EpQueue q, int64_t g0,
                                                 unsigned long long* __restrict__ stats,
                                                 uint32_t* __restrict__ err_or,
                                                 unsigned long long* __restrict__ ks) {
  const unsigned long long kt0 = kst_begin(ks);
  __shared__ __attribute__((aligned(16))) uint8_t win[(BLOCK / 64) * WIN_WAVE_BYTES];
  const LevelView lv = level_in_lds(grid, L);
  lds_u8* const wscr = (lds_u8*)win + (threadIdx.x >> 6) * WIN_WAVE_BYTES;
  step_env<AUTORESET, FINAL, POL>(S, n, L, lv.trig, lv.m, wscr, (int64_t)blockIdx.x * BLOCK + threadIdx.x,
                                  io, q, g0, stats, err_or);
  kst_end(ks, kt0);
}

// ---- two-pass compacted step (TG_MODE_COMPACT) -------------------------------------------
// Pass 1, k_classify: one lane per env (coalesced).  Evaluates option_list[a].can_run();
// envs whose option cannot run finish here (reward None, obs/done rows written, state
// unchanged); the rest are appended to per-option worklists.  Appends are aggregated per
// workgroup in LDS and the counters are sharded 8 ways (blockIdx % 8) across cache lines (one
// word alone saturates at ~88 atomics/us, MI355X_MICROARCH.md "dequeue").
// Pass 2, k_run: wave w runs chunk w (64 envs) of the worklists concatenated in run order
// (options in kRunOrder, each option's 8 shards).  Only the options are padded to whole chunks
// (round 2 padded every shard), so every wave holds ONE option: a wave-uniform k selects a loop
// specialised to that option's primitive actions.  (Round 3 also tried worklists per (option,
// predicted length class), which raised lane efficiency from 0.53 to 0.84 but ran 2-5 % slower:
// DESIGN.md §3.1.)
// worklist order = the order the chunks' loads reach HBM at the kernel's start (all option
// waves are resident at once and issue their loads together): the jump waves first, whose
// ticks are the slowest in wall time (~2,100 cycles each) and which end the kernel, then the
// long go walks (mean 56 ticks), drops, ladders, interact.  A/B against go
// first: 0.1366 vs 0.1400 ms.
// (the table is tg_dev.h's kRunOrder: the kernels index it per lane, so from constant memory)
__constant__ RunOrder kRun = kRunOrder;

// 8 waves per SIMD: its 98-106 SGPRs (the level, the step's pointers) held it to 7; forced, 32-55
// of them spill to VGPR lanes (no VGPR spills, 60 VGPRs).  A/B r04r: uniform 0.1246 vs 0.1258 ms
// per step in each of 4 rounds; masked within its spread
template <bool AUTORESET, bool FINAL, int POL = -1>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_classify(
    Soa S, int64_t n, Level L, const uint32_t* __restrict__ grid, StepIO io, EpQueue q, Work w,
    int64_t g0, unsigned long long* __restrict__ stats, uint32_t* __restrict__ err_or,
    unsigned long long* __restrict__ ks) {
  const unsigned long long kt0 = kst_begin(ks);
  __shared__ int bcnt[NLIST], bbase[NLIST];
  // stale halves per wave and the workgroup's list range: the deferred list's (k_regen) and the
  // quiet list's (this step's k_run)
  __shared__ int rwc[BLOCK / 64], rbase, qwc[BLOCK / 64], qbase;
  // the obs staging reuses the level's LDS: nothing reads the grid after the second barrier
  // below (finish_step / reset_env use only L), so 18.4 KB instead of 20.8 KB per workgroup
  __shared__ union {
    LdsLevel lv;
    double ostage[BLOCK * 9];
  } lds;
  LdsLevel& lv = lds.lv;
  double* const ostage = lds.ostage;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  const int lane = threadIdx.x & 63;
  // every load this lane may need, issued before the level staging and the barriers so their
  // latencies overlap (the angles / episode words only matter if the option cannot run)
  uint4 s4 = make_uint4(0, 0, 0, 0);
  int32_t act = 0;
  double2 a2 = make_double2(0.0, 0.0);
  int2 ep = make_int2(0, 0);
  if (live) {
    load_env<LaunchMem>(S.st4, S.ang, S.ep, i, s4, a2, ep);
    if constexpr (POL < 0) act = io.actions[i];
  }
  if (threadIdx.x < NLIST) bcnt[threadIdx.x] = 0;
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < NCTR; c += BLOCK) w.ctr_next[c * CTR_STRIDE] = 0;
  stage_cells(lv.grid, lv.trig, grid, L);  // includes the barrier
  const Map m{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H};
  Env e;
  e.mti = 0u;
  if (live) unpack_st4(s4, e);
  // the env's worklist (L_RESET's envs are reset in k_run); its stale half, for the refill list
  const auto [runs, rst, stale, bk] = classify_env<AUTORESET, POL>(L, m, e, live, act, io, i, g0 + i);
  // every env's valid row, coalesced (reward None unless its option runs; k_run writes the
  // listed envs' other rows)
  if (live) io.valid[i] = (uint8_t)runs;
  // (dense refill lists: a drain of a few steps' lists spreads one half per wave, where the
  // per-wave regions of round 4 left a wave with the few regions holding 3-4 halves for ~0.1 ms;
  // one atomic per workgroup, beside the worklists' below: per wave, ~2,000 returning atomics per
  // counter and step at the masked policy's rate serialised k_classify, 30.8 -> 39.2 us)
  // A stale half of a quiet env (live, bk < 0: no option, no L_RESET) goes on the step's quiet
  // list: nothing reads or writes that env's state word, ring or codes between this kernel and
  // the next step's k_classify except the k_run wave that claims the entry.  Any other goes on
  // the deferred list.
  const bool quiet = bk < 0;
  const unsigned long long qb = __ballot(stale && quiet), db = __ballot(stale && !quiet);
  const int srank = __popcll((quiet ? qb : db) & ((1ull << lane) - 1ull));
  if (lane == 0) {
    rwc[threadIdx.x >> 6] = __popcll(db);
    qwc[threadIdx.x >> 6] = __popcll(qb);
  }
  // workgroup-local slots: one LDS atomic per wave and list present in the wave, by the
  // group's first lane
  const auto [rank, lead, nb] = lane_groups(bk);
  int slot = 0;
  if (bk >= 0 && lane == lead) slot = atomicAdd(&bcnt[bk], nb);
  slot = __shfl(slot, lead, 64) + rank;
  __syncthreads();
  // the workgroup's worklist ranges: issue the global atomics now, use them after the
  // reward-None envs are finished (their latency overlaps that work)
  const int shard = blockIdx.x % SHARDS, wshard = blockIdx.x % WSHARDS;
  int my_base = 0;
  if (threadIdx.x < NLIST) {
    const int c = bcnt[threadIdx.x];
    my_base = c ? atomicAdd(&w.ctr[(kRun.seg_base[threadIdx.x] + wshard) * CTR_STRIDE], c) : 0;
  } else if (threadIdx.x == 64) {  // (another wave than the worklists' atomics)
    int c = 0;
#pragma unroll
    for (int v = 0; v < BLOCK / 64; ++v) c += rwc[v];
    my_base = c ? atomicAdd(&w.rcnt[shard * CTR_STRIDE], c) : 0;
  } else if (threadIdx.x == 128) {  // (and a third wave: the quiet list's)
    int c = 0;
#pragma unroll
    for (int v = 0; v < BLOCK / 64; ++v) c += qwc[v];
    my_base = c ? atomicAdd(&w.ctr[(QCTR + shard) * CTR_STRIDE], c) : 0;
  }
  const uint4 s4w = pack(e);  // the state the worklist copy carries (listed half, E_ACTION)

  // envs whose option cannot run: reward None, state unchanged (TG/:91-96, OP/:22-23); not
  // done, or auto-reset off (the others are k_run's, L_RESET)
  const bool fin = live && !runs && !rst;
  none_rows<FINAL>(L, S, fin, e, a2, i, ep, io, ostage + (threadIdx.x & ~63) * 9, err_or);
  if (fin) {
    const uint4 s4n = pack(e);
    if (s4n.x != s4.x || s4n.y != s4.y || s4n.z != s4.z || s4n.w != s4.w) {  // reset / flag
      S.st4[i] = s4n;  // (reward None: the angles, the return and the episode's start step stay)
    }
  }
  if (threadIdx.x < NLIST) bbase[threadIdx.x] = my_base;
  if (threadIdx.x == 64) rbase = my_base;
  if (threadIdx.x == 128) qbase = my_base;
  __syncthreads();
  if (stale) {
    int at = (quiet ? qbase : rbase) + srank;
    for (int v = 0; v < (int)(threadIdx.x >> 6); ++v) at += quiet ? qwc[v] : rwc[v];
    (quiet ? w.quiet + shard * w.qcap : w.refill + shard * w.rcap)[at] = refill_entry(i, e.mti);
  }
  if (bk >= 0) {
    const int64_t at = (int64_t)(kRun.seg_base[bk] + wshard) * w.shard_cap + bbase[bk] + slot;
    w.lists[at] = (int32_t)i;
    w.wst4[at] = s4w;
    w.wang[at] = a2;
    w.wep[at] = ep;
  }
  wave_stats(stats, live ? 1 : 0, runs ? 1 : 0, 0, 0, 0);
  kst_end(ks, kt0);
}

// ---- k_run's quiet drain: the step's quiet lists, by the waves that have no chunk ---------------
// k_classify lists the stale half of an env that is quiet in this step (live, in no worklist) on
// the quiet list of its shard.  Between that k_classify and the next step's, a quiet env is touched
// by nobody else: k_run's option waves read and write listed envs only, and both kernels are
// ordered on the stream with their neighbours.  So the chunk-less waves of k_run regenerate those
// halves here, under the option waves' latency chains, with k_regen's per-entry body (claim by the
// atomic AND, plain ring stores: the ring is read by later launches) at priority 0.
// Which wave takes which entry is static: the waves from the chunk space's end (`total` lanes) to
// the grid's end are numbered d = 0 .. nidle - 1, the 8 lists are concatenated, and wave d takes
// entries [d * grab, (d + 1) * grab), then strides by nidle * grab, with grab the even share (1
// for a uniform step: ~2,600 entries for > 12,000 such waves; at most 64, one per lane).  So the
// entries sit on the first chunk-less workgroups, which are dispatched right behind the option
// workgroups (numbering the waves from the grid's end, or making every 3rd or 5th chunk-less
// workgroup a draining one, measured slower than the parent: DESIGN.md §3.3).  Every
// k_run grid has nidle >= 1 (tg_dev.h RUN_EXTRA), and every wave of a grid runs, so every list is
// empty when the kernel ends, whatever the batch size, with no grab counter: 12,000 waves each
// probing 8 counters would queue at ~88 atomics / us per word, and nothing here returns a value
// through an atomic but the claims themselves.
// pre: k_run's prefix of the worklist counters; base: the wave's first lane in the grid; scr: the
// wave's code-window area (WAVE_SCRATCH bytes of it).  Returns the halves regenerated.
__device__ __forceinline__ int quiet_drain(const Soa& S, const Work& w, const int* pre, int base,
                                           lds_u32* scr, unsigned long long* __restrict__ stats) {
  __builtin_amdgcn_s_setprio(0);
  int qp[SHARDS + 1];  // the lists' exclusive prefix (wave-uniform)
  qp[0] = 0;
#pragma unroll
  for (int x = 0; x < SHARDS; ++x) qp[x + 1] = qp[x] + w.ctr[(QCTR + x) * CTR_STRIDE];
  const int64_t tot = qp[SHARDS];
  if (!tot) return 0;  // (the masked policy lists every env: nothing is quiet)
  int total = 0;  // the chunk space's end: every list padded to whole chunks
  for (int j = 0; j < NLIST; ++j) total += (pre[(j + 1) * WSHARDS] - pre[j * WSHARDS] + 63) & ~63;
  const int64_t nidle = (int64_t)gridDim.x * (RUN_BLOCK / 64) - (total >> 6);
  int64_t grab = (tot + nidle - 1) / nidle;
  if (grab > 64) grab = 64;
  const int lane = threadIdx.x & 63;
  int halves = 0;
  for (int64_t j0 = (int64_t)((base - total) >> 6) * grab; j0 < tot; j0 += nidle * grab) {
    const int64_t j = j0 + lane;
    const bool mine = lane < grab && j < tot;
    uint32_t env_l = 0u;
    if (mine) {
      int x = 0, lo = 0;  // qp[x] = lo <= j < qp[x + 1]
#pragma unroll
      for (int y = 1; y < SHARDS; ++y)
        if (j >= qp[y]) x = y, lo = qp[y];
      env_l = w.quiet[x * w.qcap + (j - lo)] & 0x7FFFFFFFu;
    }
    halves += regen_entries<false>(S, mine, env_l, scr);
  }
  if (lane == 0 && halves) {  // (k_run's grid has BLOCK / RUN_BLOCK workgroups per stats slot)
    unsigned long long* const slot = stats + (size_t)(blockIdx.x / (BLOCK / RUN_BLOCK)) * ST_COUNT;
    atomicAdd(&slot[ST_REGENS], (unsigned long long)halves);
    atomicAdd(&slot[ST_RQUIET], (unsigned long long)halves);
  }
  return halves;
}

template <bool AUTORESET, bool FINAL>
__global__ __launch_bounds__(RUN_BLOCK) void k_run(Soa S, int64_t n, Level L,
                                                const uint32_t* __restrict__ grid, StepIO io,
                                                EpQueue q, Work w, int64_t g0,
                                                unsigned long long* __restrict__ stats,
                                                uint32_t* __restrict__ err_or,
                                                unsigned long long* __restrict__ ks) {
  const unsigned long long kt0 = kst_begin(ks);
  // the worklists in run order: pre[s] = envs listed before segment s (exclusive prefix of the
  // counters, two segments per thread), then per option (run order j) its first segment's
  // prefix and its start in the chunk space, where each option is padded to whole chunks
  __shared__ int pre[NSEG + 1];
  __shared__ int wtot[RUN_BLOCK / 64];
  __shared__ int ostart[NLIST + 1], oraw[NLIST + 1];
  {
    const int s0 = 2 * (int)threadIdx.x, ln = threadIdx.x & 63;
    const int c0 = s0 < NSEG ? w.ctr[s0 * CTR_STRIDE] : 0;
    const int c1 = s0 + 1 < NSEG ? w.ctr[(s0 + 1) * CTR_STRIDE] : 0;
    int v = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(v, o, 64);
      if (ln >= o) v += y;
    }
    if (ln == 63) wtot[threadIdx.x >> 6] = v;
    __syncthreads();
    for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) v += wtot[wv];
    const int excl = v - c0 - c1;
    if (s0 < NSEG) pre[s0] = excl;
    if (s0 + 1 < NSEG) pre[s0 + 1] = excl + c0;
    if (threadIdx.x == RUN_BLOCK - 1) pre[NSEG] = v;
  }
  __syncthreads();
  const int base = (blockIdx.x * RUN_BLOCK + threadIdx.x) & ~63;  // wave w runs chunk w
  // a workgroup past every listed chunk (the grid covers n envs, a uniform step lists ~1 in 5;
  // the options' padding adds < 64 each) does not stage the level: ~3/4 of the grid
  const bool past = (int)(blockIdx.x * RUN_BLOCK) >= pre[NSEG] + NLIST * 63;
  LevelView lv{nullptr, Map{nullptr, 0, 0}, run_lds_win<RUN_BLOCK, WIN_WAVE_BYTES>()};
  if (!past) {
    if (threadIdx.x == 0) {
      int acc = 0;
      for (int j = 0; j < NLIST; ++j) {
        const int sb = j * WSHARDS, se = sb + WSHARDS;
        ostart[j] = acc;
        oraw[j] = pre[sb];
        acc += (pre[se] - pre[sb] + 63) & ~63;
      }
      ostart[NLIST] = acc;
      oraw[NLIST] = pre[NSEG];
    }
    lv = run_level_in_lds<RUN_BLOCK, WIN_WAVE_BYTES>(grid, L);  // (the barrier: ostart / oraw)
  }
  lds_u8* const wscr = (lds_u8*)lv.win + (threadIdx.x >> 6) * WIN_WAVE_BYTES;
  // A wave without a chunk (every wave of a workgroup that is past, and the last listed
  // workgroup's waves from the chunk space's end on) drains the step's quiet lists instead
  // (quiet_drain) and leaves: the option waves below never touch those lists.
  RunStamp stamp;  // the diagnostic build's per-wave timing (tg_run_diag.h): no code in the product
  stamp.begin();
  if (past || base >= ostart[NLIST]) {
    const int halves = quiet_drain(S, w, pre, base, (lds_u32*)wscr, stats);
    kst_end(ks, kt0);
    stamp.wave_end(false, 0, 0, base >> 6, halves);
    return;
  }
  const int total = ostart[NLIST];
  int oj = 0;  // ostart[oj] <= base < ostart[oj + 1] (wave-uniform)
  while (oj + 1 < NLIST && ostart[oj + 1] <= base) ++oj;
  oj = __builtin_amdgcn_readfirstlane(oj);
  const int k = kRun.list[oj];
  // this lane's place in option k's lists (the raw prefix's coordinates), and its segment
  const int qraw = oraw[oj] + base + (threadIdx.x & 63) - ostart[oj];
  const bool live = base < total && qraw < oraw[oj + 1];
  int seg = oj * WSHARDS;
  if (live) {
    int hi = seg + WSHARDS;  // pre[seg] <= qraw < pre[hi]
    while (hi - seg > 1) {
      const int mid = (seg + hi) >> 1;
      if (pre[mid] <= qraw) seg = mid; else hi = mid;
    }
  }
  const int idx = qraw - pre[seg];
  int64_t i = 0;
  StepResult r{0, 0, 0, 0};
  Env e;
  e.mti = 0u;
  int2 ep = make_int2(0, 0);
  uint32_t draws = 0;
  int lregen = 0;  // halves this lane regenerated in its option loop
  if (live) {
    const int64_t at = (int64_t)seg * w.shard_cap + idx;
    i = w.lists[at];
    load_env<LaunchMem>(w.wst4, w.wang, w.wep, at, e, ep);
    run_listed<AUTORESET, FINAL, LaunchMem>(L, lv.trig, lv.m, S, i, k, e, ep, wscr, io, err_or, r, draws,
                                        lregen, stamp);
  }
  // (k_run's grid has BLOCK / RUN_BLOCK workgroups per stats slot)
  run_epilogue<AUTORESET, LaunchMem>(S, live, i, g0 + i, e, ep, nullptr, r, draws, lregen, io.tstep, q, stats,
                                 (int64_t)blockIdx.x / (BLOCK / RUN_BLOCK));
  kst_end(ks, kt0);
  stamp.wave_end(live, k, r.ticks, base >> 6);
}

// ---- deferred regeneration of the listed stale MT halves (k_regen) ----------------------------
// k_classify appends the halves the previous step left stale (MT_STALE) to its shard's refill
// list (those of quiet envs to the step's quiet list instead: k_run's quiet drain, above) and
// marks them MT_LISTED; every REGEN_STEPS compact steps (and on tg_regenerate) k_regen
// regenerates every pending entry with a full-occupancy grid and no option loops beside it: the
// waves of XCD x (blockIdx.x % 8) take list x's entries, an even share each (the halves cost
// the same: MT_HALF_GENS twists), the rest from the list's counter.  An entry is regenerated iff
// its env's state word still says MT_STALE (its lane may have regenerated the half itself, or
// crossed again since): the half not holding the position, from the last generation of the one
// holding it.  The word loses MT_STALE | MT_LISTED by an atomic AND before the twist (the
// claim: of several entries for one env, one regenerates).  It runs alone on the stream, so
// nothing else touches the state meanwhile.
// Slack: a listed half is needed again only after the env consumes the rest of the half it is
// in, >= MT_HALF / 2 - (one step's draws) ~ 2,400 draws, more than REGEN_STEPS steps draw on the
// default level (<= ~110 per step); a lane that gets there first regenerates the half itself.
// k_regen's ring stores: non-temporal (its words and codes are read steps later, not by this
// launch) with TG_REGEN_NT=1
#ifndef TG_REGEN_NT
#define TG_REGEN_NT 0
#endif
constexpr bool REGEN_NT = TG_REGEN_NT != 0;
__global__ __launch_bounds__(BLOCK) void k_regen(Soa S, const uint32_t* __restrict__ refill,
                                                 int64_t rcap, int32_t* __restrict__ ctr,
                                                 int32_t* __restrict__ ctr_next,
                                                 unsigned long long* __restrict__ stats,
                                                 int nstat, unsigned long long* __restrict__ ks) {
  const unsigned long long kt0 = kst_begin(ks);
  __shared__ __attribute__((aligned(16))) uint32_t scratch[BLOCK / 64][MT_N];
  lds_u32* const scr = (lds_u32*)scratch[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  const int xcd = (int)(blockIdx.x & 7u);
  const int64_t cnt = ctr[(RCTR_LIST + xcd) * CTR_STRIDE];
  if (blockIdx.x == 0 && threadIdx.x < RCTR_N) ctr_next[threadIdx.x * CTR_STRIDE] = 0;
  int32_t* const q = ctr + xcd * CTR_STRIDE;
  const uint32_t* const list = refill + xcd * rcap;
  // this wave's index among its XCD's waves; the first grab is static (an even share, at most
  // 64: one entry per lane), the rest come from the counter, which starts past the static ones
  const int wx = (int)(blockIdx.x >> 3) * (BLOCK / 64) + (int)(threadIdx.x >> 6);
  const int64_t nwx = (int64_t)((gridDim.x - (unsigned)xcd + 7u) >> 3) * (BLOCK / 64);
  int64_t grab = (cnt + nwx - 1) / nwx;
  if (grab > 64) grab = 64;
  if (grab < 1) grab = 1;
  int halves = 0;
  bool first = true;
  while (true) {
    int64_t j0 = (int64_t)wx * grab;
    if (!first) {
      int g = 0;
      if (lane == 0) g = atomicAdd(q, (int)grab);
      j0 = nwx * grab + __builtin_amdgcn_readfirstlane(g);
    }
    first = false;
    if (j0 >= cnt) break;
    const int64_t m = cnt - j0 < grab ? cnt - j0 : grab;
    const uint32_t env_l = lane < m ? list[j0 + lane] & 0x7FFFFFFFu : 0u;
    halves += regen_entries<REGEN_NT>(S, lane < m, env_l, scr);  // claim, then regenerate (tg_dev.h)
  }
  // the grid can exceed the stats slots (>= 8 workgroups, one per XCD counter, at small n)
  if (lane == 0 && halves)
    atomicAdd(&stats[(size_t)(blockIdx.x % (unsigned)nstat) * ST_COUNT + ST_REGENS],
              (unsigned long long)halves);
  kst_end(ks, kt0);
}

// ---- TG_MODE_FLOW's helpers (tg_flow.h; k_flow itself is tg_flow.hip's) -----------------------
// the XCC ids the device's workgroups run on (one bit each): the flow's sub-problems
__global__ void k_census(uint32_t* mask) {
  if (threadIdx.x == 0) atomicOr(mask, 1u << (xcc_id() & 31u));
}
// after every k_flow launch, on its stream (one wave): a sub-problem whose chunks did not all
// finish step K - 1 sets TG_ERR_FLOW (no wave ran on its XCD; tg_flow.h "Coherence")
__global__ void k_flow_check(const int32_t* __restrict__ ctl, int P, int32_t C,
                             uint32_t* __restrict__ err_or) {
  const int x = (int)threadIdx.x;
  if (x < P) {
    const int Cx = (C - x + P - 1) / P;
    if (Cx > 0 && ctl[(int64_t)x * CTL_WORDS + FC_FIN * FC_STRIDE] != Cx) atomicOr(err_or, E_FLOW);
  }
}

// ---- per-env queries ----------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_mask(Soa S, int64_t n, Level L,
                                                 const uint32_t* __restrict__ grid,
                                                 uint16_t* __restrict__ out) {
  const Map m = level_in_lds(grid, L).m;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Env e;
  unpack(S.st4[i], S.ang[i], e);
  out[i] = (uint16_t)available_mask(L, m, e);
}

__global__ __launch_bounds__(BLOCK) void k_observe(Soa S, int64_t n, Level L,
                                                    double* __restrict__ obs) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Env e;
  unpack(S.st4[i], S.ang[i], e);
  double o[9];
  observe(L, e, o);
  store_obs(obs, i, o);
}

// a[t, g] = h(a0, g, t) % 9, or the k-th set bit of available_mask (masked-uniform)
__global__ __launch_bounds__(BLOCK) void k_actions(Soa S, int64_t n, Level L,
                                                    const uint32_t* __restrict__ grid,
                                                    uint64_t a0, int64_t g0, int64_t t,
                                                    int policy, int32_t* __restrict__ out) {
  __shared__ LdsLevel lv;
  if (policy == TG_POLICY_MASKED) stage_cells(lv.grid, lv.trig, grid, L);  // uniform branch
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const Map m{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H};
  Env e{};
  if (policy == TG_POLICY_MASKED) unpack(S.st4[i], S.ang[i], e);
  out[i] = policy_action(L, m, e, policy, a0, g0 + i, t);
}

// The learned actor (tg_policy_mlp.h): one env per lane.  The lane forms its obs row
// as k_observe does and keeps x, the first layer's activations and the ten head accumulators in
// VGPRs; the packed parameters sit at a wave-uniform address, so every weight is a scalar load
// into an SGPR operand of a v_fma_f32 (nothing is written through the scalar path).  masked: the
// level is staged as k_actions stages it and A is available_mask's bits.  Writes actions and,
// where given, logp, value and logits [n][9] of envs [0, n) of the view S (g0: env 0's GLOBAL
// index).  No atomics: two launches on the same state give identical bits.
template <int H, int ACT>
__global__ __launch_bounds__(BLOCK) void k_policy_mlp(Soa S, int64_t n, Level L,
                                                       const uint32_t* __restrict__ grid,
                                                       const float* __restrict__ params, int masked,
                                                       int mode, uint64_t a0, int64_t g0, int64_t t,
                                                       int32_t* __restrict__ actions,
                                                       float* __restrict__ logp,
                                                       float* __restrict__ value,
                                                       float* __restrict__ logits) {
  __shared__ LdsLevel lv;
  if (masked) stage_cells(lv.grid, lv.trig, grid, L);  // uniform branch
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const Map m{reinterpret_cast<const uint8_t*>(lv.grid), L.W, L.H};
  Env e;
  unpack(S.st4[i], S.ang[i], e);
  double o[9];
  observe(L, e, o);
  float lg[MLP_OUT], v;
  mlp_forward<H, ACT>(params, o, lg, v);
  const uint32_t allowed = mlp_allowed(masked, masked ? available_mask(L, m, e) : 0u);
  float lp;
  actions[i] = mlp_select(lg, allowed, mode, mlp_uniform(a0, g0 + i, t), lp);
  if (logp) logp[i] = lp;
  if (value) value[i] = v;
  if (logits) {
    float* q = logits + i * MLP_OUT;
#pragma unroll
    for (int k = 0; k < MLP_OUT; ++k) q[k] = lg[k];
  }
}

// move up to `cap` completed-episode records to `out`, keep the rest queued (device only,
// so the per-step episode gather never waits on the host)
__global__ __launch_bounds__(BLOCK) void k_drain_episodes(tg_episode* __restrict__ eps,
                                                           int32_t* eps_count, int32_t eps_cap,
                                                           tg_episode* __restrict__ out,
                                                           int32_t* __restrict__ count,
                                                           int32_t cap) {
  int32_t n = *eps_count;
  if ((uint32_t)n > (uint32_t)eps_cap) n = eps_cap;  // see record_episodes: never above cap + n
  const int32_t m = n < cap ? n : cap;
  for (int32_t k = threadIdx.x; k < m; k += BLOCK) out[k] = eps[k];
  __syncthreads();
  for (int32_t base = m; base < n; base += BLOCK) {  // shift the remainder down in chunks
    const int32_t k = base + threadIdx.x;
    tg_episode r;
    if (k < n) r = eps[k];
    __syncthreads();
    if (k < n) eps[k - m] = r;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *eps_count = n - m;
    *count = m;
  }
}

// The six collision predicates (IM/:232-288) at every pixel of [x0, x1) x [y0, y1) with the
// doors closed per door_bits, bit order as the reference's predicate listing: up_clear, can_go_up,
// can_go_down, can_go_left, can_go_right, can_fall.  The device build of Map (mul24 / div48
// take the __umul24 path only here), pinned against the reference's F2 truth tables.
__global__ __launch_bounds__(BLOCK) void k_predicates(Level L, const uint32_t* __restrict__ grid,
                                                       int x0, int x1, int y0, int y1,
                                                       uint32_t door_bits,
                                                       uint8_t* __restrict__ out) {
  const Map m = level_in_lds(grid, L).m;
  const int64_t w = x1 - x0;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= w * (int64_t)(y1 - y0)) return;
  Env e{};
  e.px = x0 + (int)(i % w);
  e.py = y0 + (int)(i / w);
  e.f = (door_bits & 7u) << F_OBJ;
  out[i] = (uint8_t)((unsigned)m.up_clear(e) | (unsigned)m.can_go_up(e) << 1 |
                     (unsigned)m.can_go_down(e) << 2 | (unsigned)m.can_go_side(e, -1) << 3 |
                     (unsigned)m.can_go_side(e, +1) << 4 | (unsigned)m.can_fall(e) << 5);
}

// tg_read_state's MT part: the generation holding each env's position (CPython's mt[]),
// envs [first, first + count) -> dst [count][624] (contiguous), 4 words per lane (an odd
// generation's twisted from the stored one before it: tg_snapshot.h snap_gen_quad, k_snap_save's)
__global__ __launch_bounds__(BLOCK) void k_gather_mt(Soa S, int64_t first, int64_t count,
                                                      uint32_t* __restrict__ dst) {
  constexpr int Q = MT_N / 4;  // 156 uint4 per generation
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= count * Q) return;
  const int64_t k = t / Q;
  const int q = (int)(t - k * Q);
  const int64_t i = first + k;
  reinterpret_cast<uint4*>(dst)[t] = snap_gen_quad(S.mt + i * MT_STORE, snap_gen(S.st4[i].w), q);
}

// tg_probe_dispatch: nothing (a dependent kernel boundary's cost alone)
__global__ __launch_bounds__(BLOCK) void k_null() {}

__global__ __launch_bounds__(BLOCK) void k_errors(const uint4* __restrict__ st4, int64_t n,
                                                   uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t f = i < n ? (st4_flags(st4[i]) & E_MASK) : 0u;
  if (f) atomicOr(out, f);
}

}  // namespace
