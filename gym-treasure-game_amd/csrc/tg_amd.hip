// tg_amd.hip — MI355X (gfx950) batched Treasure Game: the host code and the C ABI of
// include/tg_amd.h.  The kernels it launches are in the headers it includes: tg_dev.h (the device
// layer shared with k_flow's unit, tg_flow.hip; the state layout is described there),
// tg_kernels.h (the batch kernels), tg_timelimit.h (the step limit's kernel), tg_value_mlp.h and
// tg_gae_dev.h (the advantages' kernels), tg_py1.h (the N = 1 path) and tg_flow.h (TG_MODE_FLOW's
// types; k_flow itself is instantiated by tg_flow.hip and launched through tg::flow_launch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tg_amd.h"
#include "tg_dev.h"
#include "tg_flow.h"
#include "tg_gae_dev.h"
#include "tg_kernels.h"
#include "tg_py1.h"
#include "tg_snap_kernels.h"
#include "tg_timelimit.h"
#include "tg_value_mlp.h"

namespace tg {
thread_local std::string g_err;
std::atomic<int64_t> g_live{0};
}

namespace {

int grid_for(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }
// k_run needs one wave per 64-lane chunk of the worklists, each option padded to whole chunks:
// at most n/64 + NLIST chunks (idle blocks interleaved among the option blocks, so that MT
// regenerations start at once, measured no faster for the masked policy and slower for the
// uniform one: DESIGN.md §3.3)
int run_grid_for(int64_t n) { return grid_for(n) + (RUN_EXTRA + BLOCK - 1) / BLOCK; }
// one launch-counter slot per workgroup of the widest step launch (k_run)
int stat_slots(int64_t n) { return run_grid_for(n); }

EpQueue ep_queue(const tg_batch* h) { return EpQueue{h->eps.get(), h->eps_count.get(), h->eps_cap}; }

// ---- timing (tg_set_timing) ------------------------------------------------------------------
// The kernels of a sampled step launch (and every k_regen launch while timing is on) fold their
// in-kernel span stamps into the launch's record (kst_end): no event or other packet goes on the
// stream.  Records: KST_MAX step samples (two kernels each) and KST_MAX k_regen launches,
// KST_SLOTS slots per kernel.
constexpr int KST_MAX = 512;
constexpr int64_t KST_KSLOTS = (int64_t)KST_MAX * 3 * KST_SLOTS;  // slots of all records
unsigned long long* kst_step(Timing& T, int k, int kernel) {
  return T.kst.get() + ((size_t)k * 2 + kernel) * KST_STRIDE * KST_SLOTS;
}
unsigned long long* kst_regen(Timing& T, int k) {
  return T.kst.get() + ((size_t)KST_MAX * 2 + k) * KST_STRIDE * KST_SLOTS;
}
int kst_reset(Timing& T) {  // every record to (no start, no end)
  if (!T.kst) TG_TRY(T.kst.alloc((size_t)KST_STRIDE * KST_KSLOTS, "timing records"));
  hipLaunchKernelGGL(k_kst_init, dim3((unsigned)((KST_KSLOTS + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0,
                     T.kst.get(), KST_KSLOTS);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  T.kst_steps = 0;
  T.kst_regens = 0;
  T.kst_k.clear();
  return TG_OK;
}
// a kernel record's span in ms (first wave start to last wave end; 0 if it never ran)
double kst_span_ms(const unsigned long long* rec) {
  unsigned long long t0 = ~0ull, t1 = 0ull;
  for (int j = 0; j < KST_SLOTS; ++j) {
    if (rec[KST_STRIDE * j] < t0) t0 = rec[KST_STRIDE * j];
    if (rec[KST_STRIDE * j + 1] > t1) t1 = rec[KST_STRIDE * j + 1];
  }
  return t1 > t0 ? (double)(t1 - t0) * 1e-5 : 0.0;  // 100 MHz ticks
}
int flush_timing(Timing& T) {
  if (!T.kst_steps && !T.kst_regens) return TG_OK;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<unsigned long long> rec((size_t)KST_STRIDE * KST_KSLOTS);
  HIP_TRY(hipMemcpy(rec.data(), T.kst.get(), sizeof(unsigned long long) * rec.size(), hipMemcpyDeviceToHost));
  const size_t kr = (size_t)KST_STRIDE * KST_SLOTS;  // u64 per kernel record
  for (int k = 0; k < T.kst_steps; ++k) {
    const double c = kst_span_ms(rec.data() + (k * 2 + 0) * kr), r = kst_span_ms(rec.data() + (k * 2 + 1) * kr);
    T.sums.classify_ms += c;
    T.sums.run_ms += r;
    T.sums.kernel_ms += c + r;
    T.sums.timed_launches += k < (int)T.kst_k.size() ? T.kst_k[(size_t)k] : 1;  // k_flow: K steps
  }
  for (int k = 0; k < T.kst_regens; ++k) {
    T.sums.regen_ms += kst_span_ms(rec.data() + ((size_t)KST_MAX * 2 + k) * kr);
    ++T.sums.regen_timed;
  }
  return kst_reset(T);
}
// a step launch covering k steps: if it is sampled, ks0 / ks1 are its kernels' records (else null)
int timing_begin(Timing& T, unsigned long long*& ks0, unsigned long long*& ks1, int k = 1) {
  ks0 = ks1 = nullptr;
  if (!T.every || (T.calls++ % (uint64_t)T.every) != 0) return TG_OK;
  if (T.kst_steps >= KST_MAX) TG_TRY(flush_timing(T));
  ks0 = kst_step(T, T.kst_steps, 0);
  ks1 = kst_step(T, T.kst_steps, 1);
  ++T.kst_steps;
  T.kst_k.push_back(k);
  return TG_OK;
}

// ---- steppers (StepCtx) ----------------------------------------------------------------------
// a stepper's buffers for envs [off, off + n)
int alloc_ctx(StepCtx& c, int64_t off, int64_t n) {
  c.off = off;
  c.n = n;
  TG_TRY(c.stats.alloc(ST_COUNT * (size_t)stat_slots(n), "launch counters"));
  // a worklist shard holds the envs of every WSHARDS-th workgroup; a refill list those of every
  // SHARDS-th, REGEN_STEPS steps of them
  c.shard_cap = (int64_t)((grid_for(n) + WSHARDS - 1) / WSHARDS) * BLOCK;
  TG_TRY(c.wl.alloc(NSEG * (size_t)c.shard_cap, "worklists"));
  TG_TRY(c.wst4.alloc(NSEG * (size_t)c.shard_cap, "worklist states"));
  TG_TRY(c.wang.alloc(NSEG * (size_t)c.shard_cap, "worklist angles"));
  TG_TRY(c.wep.alloc(NSEG * (size_t)c.shard_cap, "worklist episodes"));
  TG_TRY(c.wctr.alloc(2 * NCTR * CTR_STRIDE, "worklist counters"));
  // a shard's list holds at most its workgroups' envs per pending step
  c.rcap = (int64_t)((grid_for(n) + SHARDS - 1) / SHARDS) * BLOCK * REGEN_STEPS;
  TG_TRY(c.refill.alloc(SHARDS * (size_t)c.rcap, "refill lists"));
  TG_TRY(c.regen_ctr.alloc(2 * RCTR_N * CTR_STRIDE, "k_regen counters"));
  // a quiet list holds one step's entries: drained by the k_run of the step that appended them
  c.qcap = (int64_t)((grid_for(n) + SHARDS - 1) / SHARDS) * BLOCK;
  TG_TRY(c.quiet.alloc(SHARDS * (size_t)c.qcap, "quiet lists"));
  HIP_TRY(hipMemset(c.stats.get(), 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(n)));
  HIP_TRY(hipMemset(c.wctr.get(), 0, sizeof(int32_t) * 2 * NCTR * CTR_STRIDE));
  HIP_TRY(hipMemset(c.regen_ctr.get(), 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
  return TG_OK;
}
// the handle's envs from `off` on as a Soa view (a stepper's: off = c.off)
Soa soa_of(const tg_batch* h, int64_t off) {
  return Soa{h->S.st4 + off, h->S.ang + off, h->S.ep + off, h->S.mt + off * (int64_t)MT_STORE,
             h->S.mc + off * (int64_t)MT_CODES};
}
// k_regen over the stepper's pending refill lists (its span recorded when timing is on: the
// handle's own stepper only)
int launch_regen(tg_batch* h, StepCtx& c, hipStream_t st) {
  if (!c.rpend) return TG_OK;
  unsigned long long* ks = nullptr;
  if (h->tm.every && &c == &h->main) {
    if (h->tm.kst_regens >= KST_MAX) TG_TRY(flush_timing(h->tm));
    ks = kst_regen(h->tm, h->tm.kst_regens++);
  }
  // Workgroups take list regions from the counter of their XCD (blockIdx.x % 8) until it runs
  // out, so the grid needs at least 8 of them (one per counter; fewer would leave the regions
  // of the missing counters undone) and no more than are resident at once (a second round
  // would find the counters exhausted and only pay its launch).  Block b adds its halves to
  // stats slot b % stat_slots.  The counters alternate between two sets by launch parity: each
  // launch zeroes the other set for the next one (no memset launch).
  if (!h->regen_per_cu) {
    int nb = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_regen),
                                                         BLOCK, 0));
    h->regen_per_cu = nb > 0 ? nb : 1;
  }
  // (the lists' lengths are on the device: the grid is sized for ~0.25 entries per env and step,
  // 64 per wave)
  const int64_t bound = ((c.n + 63) >> 6) * c.rpend;
  int64_t grid = (int64_t)h->cus * h->regen_per_cu;
  if (grid > (bound + 3) / 4) grid = (bound + 3) / 4;  // 4 waves per workgroup
  if (grid < 8) grid = 8;
  int32_t* const cur = c.regen_ctr.get() + c.regen_parity * RCTR_N * CTR_STRIDE;
  int32_t* const nxt = c.regen_ctr.get() + (c.regen_parity ^ 1) * RCTR_N * CTR_STRIDE;
  c.regen_parity ^= 1;
  hipLaunchKernelGGL(k_regen, dim3((unsigned)grid), dim3(BLOCK), 0, st, soa_of(h, c.off), c.refill.get(),
                     c.rcap, cur, nxt, c.stats.get(), stat_slots(c.n), ks);
  HIP_TRY(hipGetLastError());
  c.rpend = 0;
  ++h->tm.sums.regen_launches;
  return TG_OK;
}
// every stepper's pending refill lists drained on `st` (the groups' lists name halves the
// handle's own k_classify will not list again, and the reverse)
int regen_all(tg_batch* h, hipStream_t st) {
  int rc = launch_regen(h, h->main, st);
  for (auto& c : h->grp)
    if (!rc) rc = launch_regen(h, c, st);
  return rc;
}

// f(AR, FO, POL) with a step's auto-reset, final_obs and policy (-1: actions given; else the
// TG_POLICY_* evaluated in the step) as compile-time constants: the step kernels' instantiation
// for a launch
template <class F>
auto step_inst(bool ar, bool fo, int policy, F f) {
  auto with_fo = [&](auto AR, auto FO) {
    return policy == TG_POLICY_UNIFORM  ? f(AR, FO, std::integral_constant<int, TG_POLICY_UNIFORM>{})
           : policy == TG_POLICY_MASKED ? f(AR, FO, std::integral_constant<int, TG_POLICY_MASKED>{})
                                        : f(AR, FO, std::integral_constant<int, -1>{});
  };
  auto with_ar = [&](auto AR) { return fo ? with_fo(AR, std::true_type{}) : with_fo(AR, std::false_type{}); };
  return ar ? with_ar(std::true_type{}) : with_ar(std::false_type{});
}
// one step's kernels for a stepper's envs on `st` (io: the whole handle's arrays; the stepper's
// rows start at c.off), their spans sampled when timing is on (the handle's own stepper, or the
// first group).  vt (tg_rollout_mlp_gae; else null and nothing more is launched): the rollout's
// vnext rows, which get the actor's value of every env the step limit resets (need_trunc_lists
// first).
struct TruncOut {
  float* vnext;    // [steps][N]
  int64_t steps;
  int64_t row;     // this step's
};
int flush_trunc_list(tg_batch* h, StepCtx& c, const TruncOut& vt, hipStream_t st);
int launch_step(tg_batch* h, StepCtx& c, const StepIO& io_in, bool ar, hipStream_t st,
                uint32_t tstep, hipEvent_t mid = nullptr, const TruncOut* vt = nullptr) {
  StepIO io = io_in;
  io.tstep = tstep;
  if (c.off) {
    if (io.actions) io.actions += c.off;
    io.obs += c.off * 9;
    io.reward += c.off;
    io.valid += c.off;
    io.done += c.off;
    if (io.final_obs) io.final_obs += c.off * 9;
  }
  const bool fo = io.final_obs != nullptr;
  unsigned long long *ks0 = nullptr, *ks1 = nullptr;
  if (&c == &h->main || &c == h->grp.data())
    TG_TRY(timing_begin(h->tm, ks0, ks1));
  const EpQueue q = ep_queue(h);
  const dim3 grid(grid_for(c.n)), block(BLOCK);
  const Soa S = soa_of(h, c.off);
  uint32_t* const lgrid = h->grid.get();
  unsigned long long* const stats = c.stats.get();
  uint32_t* const err = h->err.get();
  const int64_t g0 = h->g0 + c.off;
  if (h->mode == TG_MODE_DIRECT) {
    const auto kern = step_inst(ar, fo, io.policy,
                                [](auto AR, auto FO, auto POL) { return &k_step<AR, FO, POL>; });
    hipLaunchKernelGGL(kern, grid, block, 0, st, S, c.n, h->L, lgrid, io, q, g0, stats, err, ks1);
  } else {
    // counters double-buffered by step parity: k_classify zeroes the next step's set (the
    // previous k_run, which read it, has finished), so no memset launch per step
    int32_t* const cur = c.wctr.get() + (c.parity ? NCTR * CTR_STRIDE : 0);
    int32_t* const nxt = c.wctr.get() + (c.parity ? 0 : NCTR * CTR_STRIDE);
    c.parity ^= 1;
    // the refill lists append until k_regen drains them (every REGEN_STEPS steps), counted in
    // the set the next k_regen reads
    const Work w{c.wl.get(), c.wst4.get(), c.wang.get(), c.wep.get(), cur, nxt, c.refill.get(),
                 c.regen_ctr.get() + (c.regen_parity * RCTR_N + RCTR_LIST) * CTR_STRIDE, c.rcap,
                 c.shard_cap, c.quiet.get(), c.qcap};
    const auto kc = step_inst(ar, fo, io.policy,
                              [](auto AR, auto FO, auto POL) { return &k_classify<AR, FO, POL>; });
    const auto kr = step_inst(ar, fo, -1, [](auto AR, auto FO, auto) { return &k_run<AR, FO>; });
    hipLaunchKernelGGL(kc, grid, block, 0, st, S, c.n, h->L, lgrid, io, q, w, g0, stats, err, ks0);
    HIP_TRY(hipGetLastError());
    if (mid) HIP_TRY(hipEventRecord(mid, st));  // (the rollouts' stagger between groups)
    hipLaunchKernelGGL(kr, dim3(run_grid_for(c.n) * (BLOCK / RUN_BLOCK)), dim3(RUN_BLOCK), 0, st, S,
                       c.n, h->L, lgrid, io, q, w, g0, stats, err, ks1);
  }
  HIP_TRY(hipGetLastError());
  if (h->mode != TG_MODE_DIRECT && ++c.rpend == REGEN_STEPS) TG_TRY(launch_regen(h, c, st));
  // the step limit (tg_set_time_limit), after everything else of the step: where a tg_reset
  // between this step and the next would stand (its block b counts in stats slot b < stat_slots)
  if (h->time_limit) {
    if (vt && ar) {  // the states k_timelimit resets, saved while they are still there
      const TruncList T{c.tst4.get(), c.tang.get(), c.tdst.get(), 4 * c.n};
      const int64_t per = (int64_t)TL_TILES * TL_BLOCK;
      hipLaunchKernelGGL(k_trunc_list, dim3((unsigned)((c.n + per - 1) / per)), dim3(TL_BLOCK), 0, st, S, c.n,
                         h->time_limit, tstep, vt->row * h->n + c.off, T, c.tcnt.get() + c.tparity,
                         c.tcnt.get() + (c.tparity ^ 1));
      HIP_TRY(hipGetLastError());
      ++c.twin;
    }
    const auto kt = ar ? &k_timelimit<true> : &k_timelimit<false>;
    hipLaunchKernelGGL(kt, grid, block, 0, st, S, c.n, h->L, h->time_limit, tstep, io.obs, io.done, q,
                       g0, stats, err);
    HIP_TRY(hipGetLastError());
    // An env truncates at most once in `limit` steps, so w steps append at most
    // n * ((w - 1) / limit + 1) entries: the list's 4 n hold 4 * limit steps.  Their values, at
    // the rollout's last step or when that bound is reached.
    if (vt && ar && (vt->row == vt->steps - 1 || c.twin >= 4 * (int64_t)h->time_limit))
      TG_TRY(flush_trunc_list(h, c, *vt, st));
  }
  return TG_OK;
}

// ---- rollouts (tg_rollout, tg_rollout_mlp) ---------------------------------------------------
// what `who` (the entry point's name) checks and prepares: the outputs, and the obs scratch
int rollout_prep(tg_batch* h, const char* who, int32_t steps, bool selector_ok, const double* obs,
                 const int32_t* reward, const uint8_t* valid, const uint8_t* done) {
  if (steps < 0 || !reward || !valid || !done || !selector_ok)
    return fail(TG_E_INVAL, "%s: bad arguments", who);
  if (!obs && !h->obs_scratch)  // the step kernels always write an obs row
    TG_TRY(h->obs_scratch.alloc(9 * (size_t)h->n, "the rollout's obs scratch"));
  return TG_OK;
}
// `steps` steps, step s being step_of(stepper, s, stream, mid): of the handle's own stepper on
// the caller's stream cs or, in compact mode with groups, of every group
template <class F>
int run_steps(tg_batch* h, int32_t steps, hipStream_t cs, F step_of) {
  int rc = TG_OK;
  if (h->grp.empty() || h->mode != TG_MODE_COMPACT) {
    for (int32_t s = 0; s < steps && !rc; ++s) rc = step_of(h->main, s, cs, (hipEvent_t) nullptr);
    return rc;
  }
  // Groups (tg_set_groups): each steps its envs on a stream of its own, so one group's
  // latency-bound k_run tail overlaps the others' bandwidth-bound k_classify / k_regen.  The
  // handle's own pending refill lists go first (the groups' k_classify would not list those
  // halves again), each group drains its own at the end, then the caller's stream joins.
  if ((rc = launch_regen(h, h->main, cs))) return rc;
  HIP_TRY(hipEventRecord(h->fork.get(), cs));
  for (auto& c : h->grp) HIP_TRY(hipStreamWaitEvent(c.st.get(), h->fork.get(), 0));
  for (int32_t s = 0; s < steps; ++s)
    for (size_t g = 0; g < h->grp.size(); ++g) {
      StepCtx& c = h->grp[g];
      // stagger: group g + 1 starts after group g's first k_classify (half a step apart)
      hipEvent_t mid = (s == 0 && h->stagger && g + 1 < h->grp.size()) ? h->grp[g + 1].ev.get() : nullptr;
      if ((rc = step_of(c, s, c.st.get(), mid))) return rc;
      if (mid) HIP_TRY(hipStreamWaitEvent(h->grp[g + 1].st.get(), mid, 0));
    }
  for (auto& c : h->grp) {
    if ((rc = launch_regen(h, c, c.st.get()))) return rc;
    HIP_TRY(hipEventRecord(c.ev.get(), c.st.get()));
    HIP_TRY(hipStreamWaitEvent(cs, c.ev.get(), 0));
  }
  return TG_OK;
}

// ---- TG_MODE_FLOW (tg_flow.h) ----------------------------------------------------------------
// the XCD census (sub-problems) and the work structures, at the first flow rollout: built
// aside and installed whole
int flow_init(tg_batch* h) {
  if (h->fl.ready) return TG_OK;
  FlowState F;
  uint32_t mask = 0;
  {
    DevBuf<uint32_t> dmask;
    TG_TRY(dmask.alloc(1, "the flow census"));
    HIP_TRY(hipMemset(dmask.get(), 0, sizeof(uint32_t)));
    // several workgroups per CU: every XCD of the device gets some (dispatch is round-robin)
    hipLaunchKernelGGL(k_census, dim3((unsigned)(h->cus * 8)), dim3(64), 0, 0, dmask.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&mask, dmask.get(), sizeof mask, hipMemcpyDeviceToHost));
  }
  mask &= 0xFFu;
  F.xmap = 0xFFFFFFFFu;
  for (int id = 0; id < 8; ++id)
    if ((mask >> id) & 1u) F.xmap = (F.xmap & ~(0xFu << (4 * id))) | ((uint32_t)F.P++ << (4 * id));
  if (F.P == 0) return fail(TG_E_HIP, "flow census: no XCC id in 0..7");
  if (h->flow_debug) fprintf(stderr, "[flow] census mask %08x P %d\n", mask, F.P);
  const int64_t C = (h->n + 63) / 64, cxm = (C + F.P - 1) / F.P;
  if (C > 0xFFFFFF) return fail(TG_E_INVAL, "flow mode: at most 2^24 chunks of 64 envs");
  F.C = (int32_t)C;
  F.lcap = cxm * 64;
  F.jcap = cxm + 1;
  F.qcap = (int64_t)FLOW_MAX_K * (2 * cxm + NLIST);  // run items + chunks to classify, per step
  const size_t nctl = (size_t)F.P * CTL_WORDS, nq = (size_t)F.P * F.qcap,
               nfill = (size_t)F.P * FLOW_MAX_K * NLIST * F.jcap,
               nlist = (size_t)F.P * FLOW_MAX_K * NLIST * F.lcap;
  for (int k = 0; k < 2; ++k) {
    TG_TRY(F.ctl[k].alloc(nctl, "flow control words"));
    TG_TRY(F.q[k].alloc(nq, "flow queues"));
    TG_TRY(F.fill[k].alloc(nfill, "flow fill counters"));
    HIP_TRY(hipMemset(F.ctl[k].get(), 0, sizeof(int32_t) * nctl));
    HIP_TRY(hipMemset(F.q[k].get(), 0xFF, sizeof(uint32_t) * nq));
    HIP_TRY(hipMemset(F.fill[k].get(), 0, sizeof(int32_t) * nfill));
  }
  TG_TRY(F.list.alloc(nlist, "flow lists"));
  TG_TRY(F.outst.alloc((size_t)C, "flow chunk states"));
  HIP_TRY(hipDeviceSynchronize());
  F.ready = true;
  h->fl = std::move(F);
  return TG_OK;
}
// k steps (<= FLOW_MAX_K) of the handle's own stepper in one k_flow launch; outputs at step s0
// of the rollout's [K][N] arrays
int launch_flow(tg_batch* h, int k, const FlowIO& io, bool ar, int pol, hipStream_t st) {
  auto& F = h->fl;
  StepCtx& c = h->main;
  // the MT slack (k_regen every REGEN_STEPS steps): drain first if these steps would overrun it
  if (c.rpend + k > REGEN_STEPS) TG_TRY(launch_regen(h, c, st));
  int& bpc = F.bpc[ar ? 1 : 0][pol ? 1 : 0];
  if (!bpc) {
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, tg::flow_kernel(ar, pol), BLOCK, 0));
    if (bpc < 1) bpc = 1;
  }
  unsigned long long *ks0 = nullptr, *ks = nullptr;  // one kernel: the record's second span, as k_run
  TG_TRY(timing_begin(h->tm, ks0, ks, k));
  const int p = F.parity;
  F.parity ^= 1;
  Flow f{F.ctl[p].get(), F.q[p].get(), F.fill[p].get(), F.list.get(), F.outst.get(),
         F.ctl[p ^ 1].get(), F.q[p ^ 1].get(), F.fill[p ^ 1].get(), c.refill.get(),
         c.regen_ctr.get() + (c.regen_parity * RCTR_N + RCTR_LIST) * CTR_STRIDE, c.rcap,
         F.qcap, F.jcap, F.lcap, F.C, F.P, k, F.xmap, h->flow_skip, nullptr, nullptr, nullptr};
#ifdef TG_FLOW_DBG
  TG_TRY(flow_diag_setup(h, f));
#endif
  if (h->flow_debug)
    fprintf(stderr, "[flow] launching k %d grid %d x %d lcap %lld qcap %lld jcap %lld C %d\n", k, h->cus, bpc,
            (long long)F.lcap, (long long)F.qcap, (long long)F.jcap, F.C);
  const FlowArgs a{h->S, h->n, h->L, h->grid.get(), io, ep_queue(h), f, h->g0, c.stats.get(),
                   stat_slots(h->n), h->err.get(), ks};
  TG_TRY(tg::flow_launch(ar, pol, (unsigned)(h->cus * bpc), st, a));
  HIP_TRY(hipGetLastError());
  ++F.launches;
  // every sub-problem's chunks finished (no XCD the census saw went without waves)
  hipLaunchKernelGGL(k_flow_check, dim3(1), dim3(64), 0, st, F.ctl[p].get(), F.P, F.C, h->err.get());
  HIP_TRY(hipGetLastError());
#ifdef TG_FLOW_DBG
  TG_TRY(flow_diag_after(h, f, k, bpc, st));
#endif
  if (h->flow_debug) {  // diagnostics: the census and every sub-problem's counters
    HIP_TRY(hipDeviceSynchronize());
    std::vector<int32_t> cw((size_t)F.P * CTL_WORDS);
    HIP_TRY(hipMemcpy(cw.data(), F.ctl[p].get(), sizeof(int32_t) * cw.size(), hipMemcpyDeviceToHost));
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, h->err.get(), sizeof err, hipMemcpyDeviceToHost));
    fprintf(stderr, "[flow] launch %lld k %d P %d xmap %08x grid %d err %08x\n", (long long)F.launches,
            k, F.P, F.xmap, h->cus * bpc, err);
    for (int x = 0; x < F.P; ++x) {
      const int32_t* c0 = cw.data() + (size_t)x * CTL_WORDS;
      fprintf(stderr, "[flow]  x %d init %d qhead %d qtail %d fin %d done %d cls", x, c0[FC_INIT * FC_STRIDE],
              c0[FC_QHEAD * FC_STRIDE], c0[FC_QTAIL * FC_STRIDE], c0[FC_FIN * FC_STRIDE], c0[FC_DONE * FC_STRIDE]);
      for (int t = 0; t < k; ++t) fprintf(stderr, " %d", c0[(FC_CLS + t) * FC_STRIDE]);
      fprintf(stderr, "\n");
    }
  }
  c.rpend += k;
  if (c.rpend >= REGEN_STEPS) return launch_regen(h, c, st);
  return TG_OK;
}

// ---- the learned actor (tg_policy_mlp.h) -----------------------------------------------------
// k_policy_mlp over envs [off, off + cnt) of the handle on `st`; the outputs are the whole
// handle's rows (the range's start at off)
int launch_policy_mlp(tg_batch* h, int64_t off, int64_t cnt, uint64_t a0, int64_t t, int mode,
                      int32_t* actions, float* logp, float* value, float* logits, hipStream_t st) {
  using K = decltype(&k_policy_mlp<16, 0>);
  static const K kern[4][2] = {{k_policy_mlp<16, 0>, k_policy_mlp<16, 1>},
                               {k_policy_mlp<32, 0>, k_policy_mlp<32, 1>},
                               {k_policy_mlp<64, 0>, k_policy_mlp<64, 1>},
                               {k_policy_mlp<128, 0>, k_policy_mlp<128, 1>}};
  const Mlp& M = h->mlp;
  const int hi = M.hidden == 16 ? 0 : M.hidden == 32 ? 1 : M.hidden == 64 ? 2 : 3;
  hipLaunchKernelGGL(kern[hi][M.act], dim3(grid_for(cnt)), dim3(BLOCK), 0, st, soa_of(h, off),
                     cnt, h->L, h->grid.get(), M.params.get(), M.masked, mode, a0, h->g0 + off, t,
                     actions + off, logp ? logp + off : nullptr, value ? value + off : nullptr,
                     logits ? logits + off * MLP_OUT : nullptr);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

// k_value_mlp: envs [off, off + cnt) of the handle into value[off ..] (T.st4 null), or the list T
// of `*count` entries, at most `bound`, into value[T.dst[k]] < total; on `st`
int launch_value_mlp(tg_batch* h, int64_t off, int64_t cnt, const TruncList& T, const int32_t* count,
                     int64_t bound, float* value, int64_t total, hipStream_t st) {
  using K = decltype(&k_value_mlp<16, 0>);
  static const K kern[4][2] = {{k_value_mlp<16, 0>, k_value_mlp<16, 1>},
                               {k_value_mlp<32, 0>, k_value_mlp<32, 1>},
                               {k_value_mlp<64, 0>, k_value_mlp<64, 1>},
                               {k_value_mlp<128, 0>, k_value_mlp<128, 1>}};
  const Mlp& M = h->mlp;
  const int hi = M.hidden == 16 ? 0 : M.hidden == 32 ? 1 : M.hidden == 64 ? 2 : 3;
  hipLaunchKernelGGL(kern[hi][M.act], dim3(grid_for(T.st4 ? bound : cnt)), dim3(BLOCK), 0, st,
                     soa_of(h, off), cnt, h->L, M.params.get(), T, count, T.st4 ? value : value + off, total);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}
// the values of the stepper's list into the rollout's vnext rows; the list's next use counts in
// the other word
int flush_trunc_list(tg_batch* h, StepCtx& c, const TruncOut& vt, hipStream_t st) {
  if (!c.twin) return TG_OK;
  const TruncList T{c.tst4.get(), c.tang.get(), c.tdst.get(), 4 * c.n};
  int64_t bound = c.n * ((c.twin - 1) / (int64_t)h->time_limit + 1);
  if (bound > T.cap) bound = T.cap;
  TG_TRY(launch_value_mlp(h, 0, 0, T, c.tcnt.get() + c.tparity, bound, vt.vnext, vt.steps * h->n, st));
  c.tparity ^= 1;
  c.twin = 0;
  return TG_OK;
}
// a stepper's list of truncated envs and its two count words (zero between uses: k_trunc_list),
// at first use; the zeroing is queued on `st`, the stream the stepper's kernels follow on.  The
// count is an int32 over at most 4 n entries, so a stepper of more than 2^28 envs is refused.
// A call that failed after a k_trunc_list and before the value kernel left entries behind
// (twin != 0): the count words are zeroed again, so none of them reaches this call's rows.
int need_trunc_lists(StepCtx& c, hipStream_t st) {
  if (c.n > ((int64_t)1 << 28))
    return fail(TG_E_INVAL, "tg_rollout_mlp_gae: more than 2^28 envs in one stepper (%lld) with a step "
                            "limit and TG_STEP_AUTORESET", (long long)c.n);
  if (c.tst4 && c.tang && c.tdst && c.tcnt) {
    if (c.twin) {
      HIP_TRY(hipMemsetAsync(c.tcnt.get(), 0, 2 * sizeof(int32_t), st));
      c.tparity = 0;
      c.twin = 0;
    }
    return TG_OK;
  }
  int rc = c.tst4.alloc(4 * (size_t)c.n, "the truncated envs' states");
  if (!rc) rc = c.tang.alloc(4 * (size_t)c.n, "the truncated envs' angles");
  if (!rc) rc = c.tdst.alloc(4 * (size_t)c.n, "the truncated envs' destinations");
  if (!rc) rc = c.tcnt.alloc(2, "the truncated envs' count");
  if (!rc && hipMemsetAsync(c.tcnt.get(), 0, 2 * sizeof(int32_t), st) != hipSuccess)
    rc = fail(TG_E_HIP, "hipMemsetAsync: the truncated envs' count");
  if (rc) {  // all or nothing: a failed call holds no more than the handle held before it
    c.tst4.reset();
    c.tang.reset();
    c.tdst.reset();
    c.tcnt.reset();
    return rc;
  }
  c.tparity = 0;
  c.twin = 0;
  return TG_OK;
}
// k_gae over the handle's n envs on `st`
int launch_gae(tg_batch* h, int32_t steps, float gamma, float lambda, const int32_t* reward,
               const uint8_t* done, const float* value, float* vnext, const float* vboot,
               int vnext_given, float* adv, float* ret, hipStream_t st) {
  const auto kern = vnext ? &k_gae<true> : &k_gae<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((h->n + GAE_BLOCK - 1) / GAE_BLOCK)), dim3(GAE_BLOCK), 0, st,
                     steps, h->n, gamma, lambda, reward, done, value, vnext, vboot, vnext_given, adv, ret);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

// ---- N = 1: the calls' buffers, the resident server (k_serve1), k_py1 ------------------------
int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
int row_out(const tg_batch* h, double* obs, int32_t* reward, uint8_t* valid, uint8_t* done) {
  const TgOne* const r = h->one.row.get();
  memcpy(obs, r->obs, sizeof r->obs);
  *reward = r->reward;
  *valid = r->valid;
  *done = r->done;
  return TG_OK;
}

// Handles whose server may be running.  At exit (the library's static destructors run before
// those of libamdhip64, which it depends on) every one still running is told to quit and waited
// for, at most a second each: no server outlives the process's pinned mailbox.
std::mutex g_srv_mu;
std::vector<tg_batch*> g_srv_handles;
void srv_register(tg_batch* h, bool live) {
  std::lock_guard<std::mutex> lk(g_srv_mu);
  auto it = std::find(g_srv_handles.begin(), g_srv_handles.end(), h);
  if (live && it == g_srv_handles.end()) g_srv_handles.push_back(h);
  if (!live && it != g_srv_handles.end()) g_srv_handles.erase(it);
}
void srv_post_quit(One& o) {
  SrvBox* const b = o.box.get();
  b->word = srv_word(SRV_QUIT, 0, false, false, 0);
  __atomic_store_n(&b->seq, ++o.seq, __ATOMIC_RELEASE);
}
struct SrvReaper {
  ~SrvReaper() {
    std::lock_guard<std::mutex> lk(g_srv_mu);
    for (tg_batch* h : g_srv_handles) {
      One& o = h->one;
      if (!o.live || hipSetDevice(h->device) != hipSuccess) continue;
      if (hipEventQuery(o.ev.get()) == hipErrorNotReady) srv_post_quit(o);
      const int64_t t0 = now_ns();
      while (hipEventQuery(o.ev.get()) == hipErrorNotReady && now_ns() - t0 < 1000000000ll) {
      }
      o.live = false;
    }
    g_srv_handles.clear();
  }
} g_srv_reaper;

// k_serve1's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the kernel
// on a device, not to a handle: it is only ever raised, to the largest size any handle's server
// has asked for there, so a handle with a smaller table never lowers it under one whose server
// will be relaunched with a larger.  False: the runtime refused the size.
std::vector<size_t> g_srv_dyn_max;  // by device (g_srv_mu)
bool srv_dyn_limit(int device, size_t dyn) {
  std::lock_guard<std::mutex> lk(g_srv_mu);
  if (g_srv_dyn_max.size() <= (size_t)device) g_srv_dyn_max.resize((size_t)device + 1, 0);
  if (dyn <= g_srv_dyn_max[device]) return true;
  if (hipFuncSetAttribute((const void*)k_serve1, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)dyn) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  g_srv_dyn_max[device] = dyn;
  return true;
}

// launch k_serve1 on the server's stream, after the work queued on the caller's stream
int srv_start(tg_batch* h, hipStream_t caller) {
  One& o = h->one;
  TG_TRY(o.need_server());
  HIP_TRY(hipEventRecord(o.dep.get(), caller));
  HIP_TRY(hipStreamWaitEvent(o.st.get(), o.dep.get(), 0));
  if (o.stage < 0) {  // the level's tables into the server's LDS, those that fit
    hipFuncAttributes fa{};
    int dev_max = 0;
    HIP_TRY(hipFuncGetAttributes(&fa, (const void*)k_serve1));
    HIP_TRY(hipDeviceGetAttribute(&dev_max, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    const size_t room = dev_max > (int)fa.sharedSizeBytes ? (size_t)dev_max - fa.sharedSizeBytes : 0;
    const size_t gb = h->L.gotab ? sizeof(uint32_t) * (size_t)h->L.W * h->L.H * 32 : 0;
    uint32_t stage = 0;
    size_t dyn = 0;
    if (gb && gb <= room) {
      stage = SRV_STAGE_GOTAB;
      dyn = gb;
    }
    if (dyn > 65536 && !srv_dyn_limit(h->device, dyn)) {
      stage = 0u;
      dyn = 0;
    }
    o.stage = (int)stage;
    o.dyn = dyn;
  }
  // whichever call launches it, a server serves every N = 1 command: nothing it may write is
  // missing (its own buffers, One::server_ready, and the handle's)
  if (!o.server_ready() || !h->S.st4 || !h->S.ang || !h->S.ep || !h->S.mt || !h->S.mc || !h->grid ||
      !h->main.stats || !h->err)
    return fail(TG_E_HIP, "k_serve1: a buffer it writes is not allocated");
  hipLaunchKernelGGL(k_serve1, dim3(1), dim3(64), o.dyn, o.st.get(), h->S, h->L, h->grid.get(),
                     o.box.dev(), o.py.dev(), o.pyc.get(), o.row.dev(), ep_queue(h), h->g0, o.idle,
                     (int)o.trace.on, (uint32_t)o.stage, h->main.stats.get(), h->err.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(o.ev.get(), o.st.get()));
  o.live = true;
  srv_register(h, true);
  o.t_last = now_ns();
  ++o.launches;
  return TG_OK;
}

// post a command and spin on its answer; a server that left (idle) before it saw the command is
// relaunched, and the new one serves it (it starts from the mailbox's done)
int srv_call(tg_batch* h, const SrvBox& c, hipStream_t caller) {
  One& o = h->one;
  // a server idle for more than half its limit (host clock, which starts after the server's)
  // may have left: ask its event before posting
  const int64_t t0 = now_ns();
  if (!o.live ||
      (t0 - o.t_last > (int64_t)o.idle * 5 && hipEventQuery(o.ev.get()) == hipSuccess)) {
    TG_TRY(srv_start(h, caller));
  }
  SrvBox* const b = o.box.get();
  const uint32_t seq = ++o.seq;
  b->word = c.word;
  b->tstep = c.tstep;
  b->gauss_bits = c.gauss_bits;
  const int64_t tp = o.trace.on ? now_ns() : 0;
  __atomic_store_n(&b->seq, seq, __ATOMIC_RELEASE);
  ++o.calls;
  for (uint64_t it = 1;; ++it) {
    if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) {
      o.t_last = now_ns();
      if (o.trace.on) {
        const double g = 10.0 * (double)(b->t_end - b->t_seen), k = (double)b->ticks;
        o.trace.post_ns += (double)(tp - t0);
        o.trace.rt_ns += (double)(o.t_last - tp);
        o.trace.gpu_ns += g;
        o.trace.fit[0] += k;
        o.trace.fit[1] += k * k;
        o.trace.fit[2] += g * k;
        if (b->phase[0]) {  // py_call's phases: pickup -> option start -> end -> observe ->
          const uint64_t t[7] = {b->t_seen, b->phase[0], b->phase[1], b->phase[2], b->phase[3],
                                 b->phase[4], b->t_end};  // barrier -> its return -> answer
          for (int j = 0; j < 6; ++j) o.trace.phase[j] += 10.0 * (double)(t[j + 1] - t[j]);
          ++o.trace.phase_n;
        }
      }
      return TG_OK;
    }
    __builtin_ia32_pause();
    if ((it & 4095) == 0) {
      const hipError_t e = hipEventQuery(o.ev.get());
      if (e == hipSuccess) {  // the server left: a new one serves the command
        if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) continue;
        TG_TRY(srv_start(h, caller));
      } else if (e != hipErrorNotReady) {
        o.live = false;
        return fail(TG_E_HIP, "tg_step1 server: %s", hipGetErrorString(e));
      } else if (now_ns() - t0 > 20000000000ll) {
        return fail(TG_E_HIP, "tg_step1 server: no answer to command %u in 20 s", seq);
      }
    }
  }
}

// one k_py1 launch (or server command): the caller's stream state in, the result row and the
// advanced state out.  The state is the 624 words, the index and (may be null: a step draws no
// gauss) has_gauss / gauss_next, wherever the caller keeps them: a tg_pystate, or the words and
// index of a CPython random.Random object (tg_step1_pywords).
template <bool RESET>
int launch_py1(tg_batch* h, int32_t action, uint32_t* words, uint32_t* index, uint32_t* has_gauss,
               double* gauss_next, hipStream_t stream) {
  if (h->n != 1 || !words || !index) return fail(TG_E_INVAL, "tg_*1_py: a 1-env handle and a stream state");
  if (*index > (uint32_t)MT_N)
    return fail(TG_E_INVAL, "tg_*1_py: index %u outside [0, 624]", *index);
  One& o = h->one;
  TG_TRY(o.need_row());
  TG_TRY(o.need_py());
  tg_pystate* const py = o.py.get();
  // the device's cached generations serve the call iff the caller's state is the one the last
  // call returned (no other draws on the stream since: the user's own, another env's)
  const bool warm = o.py_warm && *index == o.py_last.index &&
                    (!has_gauss || (*has_gauss == o.py_last.has_gauss &&
                                    memcmp(gauss_next, &o.py_last.gauss_next, sizeof(double)) == 0)) &&
                    memcmp(words, o.py_last.mt, sizeof o.py_last.mt) == 0;
  if (!warm) {
    memcpy(py->mt, words, sizeof py->mt);
    py->index = *index;
  }
  if (has_gauss) {
    py->has_gauss = *has_gauss;
    py->gauss_next = *gauss_next;
  }
  const uint32_t q0 = *index;
  const int hg = has_gauss ? (int)*has_gauss : 0;
  const double gn = has_gauss ? *gauss_next : 0.0;
  // a step's tstep is its index; a reset's, the next step's (the new episode's start)
  const uint32_t tstep = RESET ? h->tstep : h->tstep++;
  o.py_warm = false;  // until the call has returned
  if (o.serve) {
    SrvBox c{};
    c.word = srv_word(RESET ? SRV_RESET_PY : SRV_STEP_PY, action, warm, hg != 0, q0);
    c.tstep = tstep;
    memcpy(&c.gauss_bits, &gn, sizeof c.gauss_bits);
    TG_TRY(srv_call(h, c, stream));
  } else {
    hipLaunchKernelGGL(k_py1<RESET>, dim3(1), dim3(64), 0, stream, h->S, h->L, h->grid.get(), (int)action,
                       o.py.dev(), warm ? o.pyc.get() : nullptr, o.pyc.get(), q0, hg, gn, o.row.dev(), tstep,
                       h->main.stats.get(), h->err.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
  }
  memcpy(words, py->mt, sizeof py->mt);
  *index = py->index;
  memcpy(o.py_last.mt, words, sizeof o.py_last.mt);
  o.py_last.index = *index;
  if (has_gauss) {
    *has_gauss = py->has_gauss;
    *gauss_next = py->gauss_next;
    o.py_last.has_gauss = *has_gauss;
    o.py_last.gauss_next = *gauss_next;
  }
  o.py_warm = true;
  return TG_OK;
}

}  // namespace

namespace tg {
int srv_stop(tg_batch* h) {
  One& o = h->one;
  if (!o.live) return TG_OK;
  o.live = false;
  srv_register(h, false);
  if (hipEventQuery(o.ev.get()) != hipSuccess) srv_post_quit(o);
  HIP_TRY(hipEventSynchronize(o.ev.get()));
  // gone: a QUIT it left (idle) without reading is void, not a command for the next server
  o.box->done = o.box->seq;
  return TG_OK;
}
// the Python stream's state and its generations' cache on the device
int One::need_py() {
  TG_TRY(py.alloc("Python stream state"));
  if (!pyc) {
    TG_TRY(pyc.alloc((size_t)PY_GENS * MT_N, "Python stream cache"));
    py_warm = false;
  }
  return TG_OK;
}
// (the stream state is the server's kernel argument; only SRV_*_PY commands touch it)
int One::need_server() {
  TG_TRY(need_row());
  TG_TRY(need_py());
  if (!box) seq = 0;
  TG_TRY(box.alloc("server mailbox"));
  TG_TRY(st.create());
  TG_TRY(ev.create());
  return dep.create();
}
}  // namespace tg

extern "C" {

// ---- lifecycle and settings ------------------------------------------------------------------
const char* tg_last_error(void) { return tg::g_err.c_str(); }
const char* tg_version(void) { return "tg_amd 0.1 gfx950"; }
int64_t tg_num_envs(const tg_batch* h) { return h ? h->n : 0; }

int tg_create(tg_batch** out, int64_t n, uint64_t seed_base, int64_t global_offset, int device,
              const char* dom, const char* objs, const char* inter) {
  if (!out || n <= 0 || global_offset < 0) return fail(TG_E_INVAL, "tg_create: bad arguments");
  // every env's seed seed_base + global_offset + i must be a 64-bit init_by_array key
  if ((uint64_t)global_offset > ~seed_base || (uint64_t)(n - 1) > ~(seed_base + (uint64_t)global_offset))
    return fail(TG_E_INVAL, "tg_create: seed_base + global_offset + num_envs - 1 exceeds 2^64 - 1");
  *out = nullptr;
  if (!dom && !objs && !inter) {
    dom = kDefaultDomain;
    objs = kDefaultObjects;
    inter = kDefaultInteractions;
  } else if (!dom || !objs || !inter) {
    return fail(TG_E_INVAL, "tg_create: give all three level texts or none");
  }
  Level L;
  std::vector<uint8_t> grid;
  std::string perr;
  if (parse_level(dom, objs, inter, L, grid, perr)) return fail(TG_E_INVAL, "%s", perr.c_str());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(TG_E_NODEV, "tg_create: no HIP device %d (found %d)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TG_E_NODEV, "tg_create: device %d is %s, this build targets gfx950", device,
                prop.gcnArchName);

  std::unique_ptr<tg_batch, decltype(&tg_destroy)> hold(new tg_batch(), &tg_destroy);
  tg_batch* const h = hold.get();  // (a return before the end destroys it, and all it holds)
  h->device = device;
  h->cus = prop.multiProcessorCount;
  h->n = n;
  h->g0 = global_offset;
  h->seed0 = seed_base;
  h->domain = dom;
  h->flow_debug = getenv("TG_FLOW_DEBUG") != nullptr;
  if (const char* sp = getenv("TG_FLOW_SKIP_PART")) h->flow_skip = atoi(sp);
  if (const char* sv = getenv("TG_SERVE")) h->one.serve = atoi(sv) != 0;
  h->one.trace.on = getenv("TG_SERVE_TRACE") != nullptr;
  // the server's idle limit: 500 us by default (a stream it shares a hardware queue with waits
  // at most this long behind it)
  const char* si = getenv("TG_SERVE_IDLE_US");
  h->one.idle = 100u * (uint32_t)std::min(std::max(si ? atoi(si) : 500, 1), 1000000);
  // completed-episode queue: drained by tg_episodes; records beyond it are counted as dropped
  const int64_t cap = 4 * n > (1 << 16) ? 4 * n : (1 << 16);
  h->eps_cap = (int32_t)(cap < (1 << 28) ? cap : (1 << 28));
  uint32_t gen[MT_N];
  genrand_prefix(gen);
  grid.resize((grid.size() + 3) & ~(size_t)3, 0);
  const std::vector<uint32_t> gotab = build_gotab(L, grid);
  const std::vector<uint32_t> masks = build_masks(L, grid);
  const std::vector<double> obs_q = build_obs_q(L);
  TG_TRY(h->grid.upload(grid.data(), grid.size() / 4, "the level grid"));
  TG_TRY(h->genrand.upload(gen, MT_N, "the seeding prefix"));
  TG_TRY(h->gotab.upload(gotab.data(), gotab.size(), "the GoTable"));
  if (!masks.empty()) TG_TRY(h->masks.upload(masks.data(), masks.size(), "the level bitmasks"));
  TG_TRY(h->obs_q.upload(obs_q.data(), obs_q.size(), "the obs quotient table"));
  TG_TRY(h->env.st4.alloc((size_t)n, "env states"));
  TG_TRY(h->env.ang.alloc((size_t)n, "env angles"));
  TG_TRY(h->env.ep.alloc((size_t)n, "env episodes"));
  TG_TRY(h->env.mt.alloc(MT_STORE * (size_t)n, "env MT rings"));
  TG_TRY(h->env.mc.alloc(MT_CODES * (size_t)n, "env draw codes"));
  h->S = Soa{h->env.st4.get(), h->env.ang.get(), h->env.ep.get(), h->env.mt.get(), h->env.mc.get()};
  TG_TRY(h->eps.alloc((size_t)h->eps_cap, "the episode queue"));
  TG_TRY(h->eps_count.alloc(1, "the episode count"));
  TG_TRY(h->err.alloc(1, "the error word"));
  TG_TRY(alloc_ctx(h->main, 0, n));
  L.gotab = h->gotab.get();
  L.masks = h->masks.get();
  L.obs_q = h->obs_q.get();
  h->L = L;
  HIP_TRY(hipMemset(h->eps_count.get(), 0, sizeof(int32_t)));
  HIP_TRY(hipMemset(h->err.get(), 0, sizeof(uint32_t)));
  // seed -> generation 1 (first half) -> generation 2 (second half) -> the constructor's draws
  hipLaunchKernelGGL(k_create, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n,
                     seed_base + (uint64_t)global_offset, h->genrand.get());
  hipLaunchKernelGGL(k_gen_twist, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n,
                     MT_SEED_OFF, 0, 2 * MT_HALF_GENS);
  hipLaunchKernelGGL(k_reset, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n, h->L,
                     (const uint8_t*)nullptr, (double*)nullptr, 0u);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(TG_E_HIP, "k_create: %s", hipGetErrorString(e));
  *out = hold.release();
  return TG_OK;
}

void tg_destroy(tg_batch* h) {
  if (!h) return;
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != h->device) (void)hipSetDevice(h->device);
  (void)srv_stop(h);
  srv_register(h, false);
  const One& o = h->one;
  if (o.trace.on && o.calls)
    fprintf(stderr, "[serve] calls %lld launches %lld: mean per call %.2f us to post, %.2f us post -> "
            "answer, of which %.2f us between the server's pickup and its answer\n",
            (long long)o.calls, (long long)o.launches, o.trace.post_ns / o.calls / 1e3,
            o.trace.rt_ns / o.calls / 1e3, o.trace.gpu_ns / o.calls / 1e3);
  if (o.trace.on && o.calls > 2) {  // server time = a + b * ticks (least squares)
    const double n = (double)o.calls, sk = o.trace.fit[0], skk = o.trace.fit[1];
    const double sg = o.trace.gpu_ns, sgk = o.trace.fit[2];
    const double b = (n * sgk - sk * sg) / (n * skk - sk * sk), a = (sg - b * sk) / n;
    fprintf(stderr, "[serve] ticks per command %.2f; server time = %.2f us + %.3f us x ticks "
            "(GoTable in LDS: %d, %zu B)\n", sk / n, a / 1e3, b / 1e3, o.stage, o.dyn);
    if (o.trace.phase_n)
      fprintf(stderr, "[serve] py steps %lld, mean us: pickup -> option %.3f, option %.3f, observe "
              "%.3f, -> barrier %.3f, -> py_call return %.3f, -> answer %.3f\n",
              (long long)o.trace.phase_n, o.trace.phase[0] / o.trace.phase_n / 1e3,
              o.trace.phase[1] / o.trace.phase_n / 1e3, o.trace.phase[2] / o.trace.phase_n / 1e3,
              o.trace.phase[3] / o.trace.phase_n / 1e3, o.trace.phase[4] / o.trace.phase_n / 1e3,
              o.trace.phase[5] / o.trace.phase_n / 1e3);
  }
  delete h;  // every buffer, stream and event: by its owner
}

int tg_set_mode(tg_batch* h, int mode, int run_blocks) {
  BIND(h);
  if (mode != TG_MODE_DIRECT && mode != TG_MODE_COMPACT && mode != TG_MODE_FLOW)
    return fail(TG_E_INVAL, "tg_set_mode: unknown mode %d", mode);
  if (mode == TG_MODE_FLOW && !h->grp.empty())
    return fail(TG_E_INVAL, "tg_set_mode: TG_MODE_FLOW steps the whole batch in one k_flow launch; "
                            "call tg_set_groups(h, 1, 0) first");
  h->mode = mode;
  (void)run_blocks;  // reserved
  return TG_OK;
}

int tg_set_groups(tg_batch* h, int32_t groups, int32_t stagger) {
  BIND(h);
  if (groups > 1 && h->mode == TG_MODE_FLOW)
    return fail(TG_E_INVAL, "tg_set_groups: groups are a TG_MODE_COMPACT rollout form (TG_MODE_FLOW "
                            "steps the whole batch in one k_flow launch)");
  if (groups < 1 || groups > 16 || (int64_t)groups * 4096 > h->n)
    return fail(TG_E_INVAL, "tg_set_groups: %d groups of %lld envs (1..16, >= 4096 envs each)",
                groups, (long long)h->n);
  HIP_TRY(hipDeviceSynchronize());
  TG_TRY(regen_all(h, 0));  // the old groups' pending lists
  HIP_TRY(hipDeviceSynchronize());
  // the new groups, complete before they replace the old: contiguous groups of whole 256-env
  // workgroups, each with a stream and a join event
  std::vector<StepCtx> grp((size_t)(groups > 1 ? groups : 0));
  const int64_t per = ((h->n + groups - 1) / groups + BLOCK - 1) / BLOCK * BLOCK;
  for (size_t g = 0; g < grp.size(); ++g) {
    const int64_t off = per * (int64_t)g, cnt = std::min(per, h->n - off);
    if (cnt <= 0) return fail(TG_E_INVAL, "tg_set_groups: empty group");
    TG_TRY(alloc_ctx(grp[g], off, cnt));
    TG_TRY(grp[g].st.create());
    TG_TRY(grp[g].ev.create());
  }
  if (!grp.empty()) TG_TRY(h->fork.create());
  if (!h->grp.empty()) {  // the old groups' launch counters go on with the handle's own
    std::vector<unsigned long long> slot0(ST_COUNT);
    HIP_TRY(hipMemcpy(slot0.data(), h->main.stats.get(), sizeof(unsigned long long) * ST_COUNT,
                      hipMemcpyDeviceToHost));
    for (auto& c : h->grp) {
      std::vector<unsigned long long> part((size_t)stat_slots(c.n) * ST_COUNT);
      HIP_TRY(hipMemcpy(part.data(), c.stats.get(), sizeof(unsigned long long) * part.size(),
                        hipMemcpyDeviceToHost));
      for (size_t i = 0; i < part.size(); ++i) slot0[i % ST_COUNT] += part[i];
    }
    HIP_TRY(hipMemcpy(h->main.stats.get(), slot0.data(), sizeof(unsigned long long) * ST_COUNT,
                      hipMemcpyHostToDevice));
  }
  h->grp = std::move(grp);
  h->stagger = stagger != 0;
  return TG_OK;
}

int tg_set_time_limit(tg_batch* h, int32_t max_steps) {
  BIND(h);
  if (max_steps < 0 || max_steps >= TG_EPISODE_TRUNCATED)
    return fail(TG_E_INVAL, "tg_set_time_limit: max_steps %d (0 = off, 1 .. 2^30 - 1)", max_steps);
  h->time_limit = (uint32_t)max_steps;
  return TG_OK;
}

int tg_set_episode_capacity(tg_batch* h, int32_t cap) {
  BIND(h);
  if (cap < 1 || cap > (1 << 28)) return fail(TG_E_INVAL, "tg_set_episode_capacity: cap %d", cap);
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<tg_episode> eps;  // (the old queue stays if the new one cannot be had)
  TG_TRY(eps.alloc((size_t)cap, "the episode queue"));
  h->eps = std::move(eps);
  h->eps_cap = cap;
  HIP_TRY(hipMemset(h->eps_count.get(), 0, sizeof(int32_t)));
  return TG_OK;
}

// ---- reset, step and rollout -----------------------------------------------------------------
int tg_reset(tg_batch* h, const uint8_t* mask, double* obs, void* stream) {
  BIND(h);
  hipLaunchKernelGGL(k_reset, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, mask, obs, h->tstep);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_step(tg_batch* h, const int32_t* actions, double* obs, int32_t* reward, uint8_t* valid,
            uint8_t* done, double* final_obs, uint32_t flags, void* stream) {
  BIND(h);
  if (!actions || !obs || !reward || !valid || !done)
    return fail(TG_E_INVAL, "tg_step: actions/obs/reward/valid/done are required");
  const StepIO io{const_cast<int32_t*>(actions), obs, reward, valid, done, final_obs, -1, 0, 0};
  return launch_step(h, h->main, io, (flags & TG_STEP_AUTORESET) != 0, (hipStream_t)stream,
                     h->tstep++);
}

int tg_rollout(tg_batch* h, int32_t steps, uint64_t action_seed, int64_t t0, int policy,
               uint32_t flags, int32_t* actions, double* obs, int32_t* reward, uint8_t* valid,
               uint8_t* done, void* stream) {
  BIND(h);
  if (h->mode == TG_MODE_FLOW && h->time_limit)
    return fail(TG_E_INVAL, "tg_rollout: TG_MODE_FLOW runs its steps inside k_flow, which has no step "
                            "boundary for tg_set_time_limit's limit; use TG_MODE_COMPACT or "
                            "TG_MODE_DIRECT, or tg_step");
  if (steps == 0) return TG_OK;
  TG_TRY(rollout_prep(h, "tg_rollout", steps, policy == TG_POLICY_UNIFORM || policy == TG_POLICY_MASKED,
                      obs, reward, valid, done));
  const int64_t n = h->n;
  const bool ar = (flags & TG_STEP_AUTORESET) != 0;
  hipStream_t cs = (hipStream_t)stream;
  const uint32_t tb = h->tstep;
  h->tstep += (uint32_t)steps;
  if (h->mode == TG_MODE_FLOW) {  // k_flow, up to FLOW_MAX_K steps per launch (no groups: tg_set_mode)
    int rc = flow_init(h);
    for (int32_t s = 0; s < steps && !rc; s += FLOW_MAX_K) {
      const int k = steps - s < FLOW_MAX_K ? steps - s : FLOW_MAX_K;
      const FlowIO io{actions ? actions + (size_t)s * n : nullptr,
                      obs ? obs + (size_t)s * n * 9 : h->obs_scratch.get(), obs ? n * 9 : 0,
                      reward + (size_t)s * n, valid + (size_t)s * n, done + (size_t)s * n,
                      action_seed, t0 + s, tb + (uint32_t)s};
      rc = launch_flow(h, k, io, ar, policy == TG_POLICY_MASKED ? 1 : 0, cs);
    }
    return rc;
  }
  return run_steps(h, steps, cs, [&](StepCtx& c, int32_t s, hipStream_t st, hipEvent_t mid) {
    const StepIO io{actions ? actions + (size_t)s * n : nullptr,
                    obs ? obs + (size_t)s * n * 9 : h->obs_scratch.get(),
                    reward + (size_t)s * n, valid + (size_t)s * n, done + (size_t)s * n,
                    nullptr, policy, action_seed, t0 + s};
    return launch_step(h, c, io, ar, st, tb + (uint32_t)s, mid);
  });
}

int tg_regenerate(tg_batch* h, void* stream) {
  BIND(h);
  return regen_all(h, (hipStream_t)stream);
}

// ---- N = 1 (served by k_serve1 when the server is on) ----------------------------------------
int tg_step1(tg_batch* h, int32_t action, double* obs, int32_t* reward, uint8_t* valid,
             uint8_t* done, void* stream) {
  BIND_SERVE(h);
  if (h->n != 1 || !obs || !reward || !valid || !done)
    return fail(TG_E_INVAL, "tg_step1: a 1-env handle and host obs/reward/valid/done");
  TG_TRY(h->one.need_row());
  hipStream_t st = (hipStream_t)stream;
  if (h->one.serve) {
    SrvBox c{};
    c.word = srv_word(SRV_STEP, action, false, false, 0);
    c.tstep = h->tstep++;
    TG_TRY(srv_call(h, c, st));
  } else {
    TgOne* const d = h->one.row.dev();
    const StepIO io{nullptr, d->obs, &d->reward, &d->valid, &d->done, nullptr, POL_IMMEDIATE,
                    (uint64_t)(int64_t)action, 0, h->tstep++};
    hipLaunchKernelGGL((k_step<false, false, POL_IMMEDIATE>), dim3(1), dim3(BLOCK), 0, st, h->S,
                       h->n, h->L, h->grid.get(), io, ep_queue(h), h->g0, h->main.stats.get(),
                       h->err.get(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  return row_out(h, obs, reward, valid, done);
}

int tg_available_mask1(tg_batch* h, uint16_t* mask, void* stream) {
  BIND_SERVE(h);
  if (h->n != 1 || !mask) return fail(TG_E_INVAL, "tg_available_mask1: a 1-env handle and a host output");
  One& o = h->one;
  if (o.serve) {
    SrvBox c{};
    c.word = srv_word(SRV_MASK, 0, false, false, 0);
    TG_TRY(srv_call(h, c, (hipStream_t)stream));
    *mask = (uint16_t)o.box->mask;
    return TG_OK;
  }
  TG_TRY(o.mask1.alloc("tg_available_mask1's result"));
  hipLaunchKernelGGL(k_mask, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->S, h->n, h->L,
                     h->grid.get(), o.mask1.dev());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *mask = *o.mask1.get();
  return TG_OK;
}

int tg_reset1(tg_batch* h, double* obs, void* stream) {
  BIND_SERVE(h);
  if (h->n != 1) return fail(TG_E_INVAL, "tg_reset1: a 1-env handle");
  if (h->one.serve) {
    SrvBox c{};
    c.word = srv_word(SRV_RESET, 0, false, false, 0);
    c.tstep = h->tstep;  // the next step's index: the new episode's start (as tg_reset)
    TG_TRY(srv_call(h, c, (hipStream_t)stream));
  } else {
    TG_TRY(h->one.need_row());
    hipLaunchKernelGGL(k_reset, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->S, h->n, h->L,
                       (const uint8_t*)nullptr, h->one.row.dev()->obs, h->tstep);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  if (obs) memcpy(obs, h->one.row->obs, sizeof h->one.row->obs);
  return TG_OK;
}

int tg_set_serve(tg_batch* h, int on) {
  BIND(h);  // (stops a running server)
  h->one.serve = on != 0;
  return TG_OK;
}

int tg_step1_py(tg_batch* h, int32_t action, tg_pystate* st, double* obs, int32_t* reward,
                uint8_t* valid, uint8_t* done, void* stream) {
  BIND_SERVE(h);
  if (!obs || !reward || !valid || !done || !st) return fail(TG_E_INVAL, "tg_step1_py: null output");
  const int rc = launch_py1<false>(h, action, st->mt, &st->index, &st->has_gauss, &st->gauss_next,
                                   (hipStream_t)stream);
  return rc ? rc : row_out(h, obs, reward, valid, done);
}

int tg_step1_pywords(tg_batch* h, int32_t action, uint32_t* words, int32_t* index, double* obs,
                     int32_t* reward, uint8_t* valid, uint8_t* done, void* stream) {
  BIND_SERVE(h);
  if (!obs || !reward || !valid || !done || !words || !index)
    return fail(TG_E_INVAL, "tg_step1_pywords: null argument");
  if (*index < 0) return fail(TG_E_INVAL, "tg_step1_pywords: index %d < 0", *index);
  const int rc = launch_py1<false>(h, action, words, reinterpret_cast<uint32_t*>(index), nullptr,
                                   nullptr, (hipStream_t)stream);
  return rc ? rc : row_out(h, obs, reward, valid, done);
}

int tg_reset1_py(tg_batch* h, tg_pystate* st, double* obs, void* stream) {
  BIND_SERVE(h);
  if (!st) return fail(TG_E_INVAL, "tg_reset1_py: null stream state");
  const int rc = launch_py1<true>(h, 0, st->mt, &st->index, &st->has_gauss, &st->gauss_next,
                                  (hipStream_t)stream);
  if (rc) return rc;
  if (obs) memcpy(obs, h->one.row->obs, sizeof h->one.row->obs);
  return TG_OK;
}

// ---- policies --------------------------------------------------------------------------------
int tg_policy_actions(tg_batch* h, uint64_t a0, int64_t t, int policy, int32_t* actions,
                      void* stream) {
  BIND(h);
  if (!actions || (policy != TG_POLICY_UNIFORM && policy != TG_POLICY_MASKED))
    return fail(TG_E_INVAL, "tg_policy_actions: bad arguments");
  hipLaunchKernelGGL(k_actions, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, h->grid.get(), a0, h->g0, t, policy, actions);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_policy_mlp_load(tg_batch* h, int32_t hidden, int32_t act, int32_t masked,
                       const float* params_dev, void* stream) {
  BIND(h);
  if (!mlp_hidden_ok(hidden) || (act != TG_ACT_RELU && act != TG_ACT_TANH) || !params_dev)
    return fail(TG_E_INVAL, "tg_policy_mlp_load: hidden %d (16, 32, 64, 128), act %d (TG_ACT_*) and "
                            "a device pointer to the packed parameters", hidden, act);
  // sized once for the widest network, so a later load never reallocates (or synchronises)
  Mlp& M = h->mlp;
  if (!M.params) TG_TRY(M.params.alloc((size_t)mlp_param_count(MLP_MAX_HIDDEN), "the actor's parameters"));
  HIP_TRY(hipMemcpyAsync(M.params.get(), params_dev, sizeof(float) * (size_t)mlp_param_count(hidden),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  M.hidden = hidden;
  M.act = act;
  M.masked = masked ? 1 : 0;
  return TG_OK;
}

int tg_policy_mlp(tg_batch* h, uint64_t a0, int64_t t, int32_t mode, int32_t* actions, float* logp,
                  float* value, float* logits, void* stream) {
  BIND(h);
  if (!h->mlp.hidden) return fail(TG_E_STATE, "tg_policy_mlp: no parameters (tg_policy_mlp_load)");
  if (!actions || (mode != TG_MLP_SAMPLE && mode != TG_MLP_GREEDY))
    return fail(TG_E_INVAL, "tg_policy_mlp: bad arguments");
  return launch_policy_mlp(h, 0, h->n, a0, t, mode, actions, logp, value, logits,
                           (hipStream_t)stream);
}

}  // extern "C"

namespace {
// tg_rollout_mlp (vnext null) and tg_rollout_mlp_gae's rollout (`who`): with vnext, a limit and
// auto-reset, row s of vnext gets the value of every env the limit resets in step s
int rollout_mlp(tg_batch* h, const char* who, int32_t steps, uint64_t a0, int64_t t0, int32_t mode,
                uint32_t flags, int32_t* actions, double* obs, int32_t* reward, uint8_t* valid,
                uint8_t* done, float* logp, float* value, float* vnext, bool own_vboot, void* stream) {
  if (!h->mlp.hidden) return fail(TG_E_STATE, "%s: no parameters (tg_policy_mlp_load)", who);
  if (h->mode == TG_MODE_FLOW)
    return fail(TG_E_INVAL, "%s: TG_MODE_FLOW evaluates its policy inside k_flow; use "
                            "TG_MODE_COMPACT or TG_MODE_DIRECT", who);
  if (steps == 0) return TG_OK;
  TG_TRY(rollout_prep(h, who, steps, mode == TG_MLP_SAMPLE || mode == TG_MLP_GREEDY, obs,
                      reward, valid, done));
  const int64_t n = h->n;
  if (!actions && !h->mlp.actions)  // the step kernels always read an action row
    TG_TRY(h->mlp.actions.alloc((size_t)n, "tg_rollout_mlp's action scratch"));
  if (own_vboot && !h->mlp.vboot) TG_TRY(h->mlp.vboot.alloc((size_t)n, "tg_rollout_mlp_gae's vboot scratch"));
  const bool ar = (flags & TG_STEP_AUTORESET) != 0;
  if (vnext && ar && h->time_limit) {  // every stepper run_steps will use
    if (h->grp.empty() || h->mode != TG_MODE_COMPACT) {
      TG_TRY(need_trunc_lists(h->main, (hipStream_t)stream));
    } else {
      for (auto& c : h->grp) TG_TRY(need_trunc_lists(c, c.st.get()));
    }
  }
  const uint32_t tb = h->tstep;
  h->tstep += (uint32_t)steps;
  // step s of a stepper: the actor into row s, then the step kernels with those actions given
  return run_steps(h, steps, (hipStream_t)stream,
                   [&](StepCtx& c, int32_t s, hipStream_t st, hipEvent_t mid) {
    int32_t* const act = actions ? actions + (size_t)s * n : h->mlp.actions.get();
    const int rc = launch_policy_mlp(h, c.off, c.n, a0, t0 + s, mode, act,
                                     logp ? logp + (size_t)s * n : nullptr,
                                     value ? value + (size_t)s * n : nullptr, nullptr, st);
    if (rc) return rc;
    const StepIO io{act, obs ? obs + (size_t)s * n * 9 : h->obs_scratch.get(), reward + (size_t)s * n,
                    valid + (size_t)s * n, done + (size_t)s * n, nullptr, -1, 0, 0};
    const TruncOut vt{vnext, steps, s};
    return launch_step(h, c, io, ar, st, tb + (uint32_t)s, mid, vnext ? &vt : nullptr);
  });
}
}  // namespace

extern "C" {

int tg_rollout_mlp(tg_batch* h, int32_t steps, uint64_t a0, int64_t t0, int32_t mode, uint32_t flags,
                   int32_t* actions, double* obs, int32_t* reward, uint8_t* valid, uint8_t* done,
                   float* logp, float* value, void* stream) {
  BIND(h);
  return rollout_mlp(h, "tg_rollout_mlp", steps, a0, t0, mode, flags, actions, obs, reward, valid, done,
                     logp, value, nullptr, false, stream);
}

// ---- advantages (tg_gae.h) -------------------------------------------------------------------
int tg_gae(tg_batch* h, int32_t steps, float gamma, float lambda, const int32_t* reward,
           const uint8_t* done, const float* value, float* vnext, const float* vboot,
           int32_t vnext_given, float* adv, float* ret, void* stream) {
  BIND(h);
  if (!gae_coeff_ok(gamma) || !gae_coeff_ok(lambda))
    return fail(TG_E_INVAL, "tg_gae: gamma %g and lambda %g must lie in [0, 1]", (double)gamma, (double)lambda);
  if (steps == 0) return TG_OK;  // (rows of no steps have no address)
  if (steps < 0 || !reward || !done || !value || !vboot || !adv || !ret || (vnext_given && !vnext))
    return fail(TG_E_INVAL, "tg_gae: bad arguments");
  return launch_gae(h, steps, gamma, lambda, reward, done, value, vnext, vboot, vnext_given ? 1 : 0, adv,
                    ret, (hipStream_t)stream);
}

int tg_rollout_mlp_gae(tg_batch* h, int32_t steps, uint64_t a0, int64_t t0, int32_t mode, uint32_t flags,
                       int32_t* actions, double* obs, int32_t* reward, uint8_t* valid, uint8_t* done,
                       float* logp, float* value, float gamma, float lambda, float* adv, float* ret,
                       float* vnext, float* vboot, void* stream) {
  BIND(h);
  if (!gae_coeff_ok(gamma) || !gae_coeff_ok(lambda))
    return fail(TG_E_INVAL, "tg_rollout_mlp_gae: gamma %g and lambda %g must lie in [0, 1]", (double)gamma,
                (double)lambda);
  if (!adv || !ret || !value) return fail(TG_E_INVAL, "tg_rollout_mlp_gae: adv, ret and value are required");
  const bool parks = h->time_limit && (flags & TG_STEP_AUTORESET);  // the truncated values, in vnext
  if (parks && !vnext)
    return fail(TG_E_INVAL, "tg_rollout_mlp_gae: with a step limit and TG_STEP_AUTORESET vnext is required "
                            "(the truncated envs' values are parked there)");
  TG_TRY(rollout_mlp(h, "tg_rollout_mlp_gae", steps, a0, t0, mode, flags, actions, obs, reward, valid, done,
                     logp, value, vnext, !vboot, stream));
  if (steps == 0) return TG_OK;
  // (with groups, the caller's stream has joined them: run_steps)
  float* const vb = vboot ? vboot : h->mlp.vboot.get();
  TG_TRY(launch_value_mlp(h, 0, h->n, TruncList{}, nullptr, 0, vb, h->n, (hipStream_t)stream));
  return launch_gae(h, steps, gamma, lambda, reward, done, value, vnext, vb, parks ? 1 : 0, adv, ret,
                    (hipStream_t)stream);
}

// ---- state in and out ------------------------------------------------------------------------
int tg_available_mask(tg_batch* h, uint16_t* mask, void* stream) {
  BIND(h);
  if (!mask) return fail(TG_E_INVAL, "tg_available_mask: null output");
  hipLaunchKernelGGL(k_mask, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, h->grid.get(), mask);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_observe(tg_batch* h, double* obs, void* stream) {
  BIND(h);
  if (!obs) return fail(TG_E_INVAL, "tg_observe: null output");
  hipLaunchKernelGGL(k_observe, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, obs);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_episodes(tg_batch* h, tg_episode* out, int32_t* count, int32_t cap, void* stream) {
  BIND(h);
  if (!out || !count || cap < 0) return fail(TG_E_INVAL, "tg_episodes: bad arguments");
  hipLaunchKernelGGL(k_drain_episodes, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->eps.get(),
                     h->eps_count.get(), h->eps_cap, out, count, cap);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_read_state(tg_batch* h, int32_t* pos, uint32_t* flags, int32_t* objs, double* ang,
                  uint32_t* mt, uint32_t* mt_pos, int32_t* ep) {
  BIND(h);
  HIP_TRY(hipDeviceSynchronize());
  const int64_t n = h->n;
  std::vector<uint4> st;
  if (pos || flags || objs || mt || mt_pos) {
    st.resize((size_t)n);
    HIP_TRY(hipMemcpy(st.data(), h->S.st4, sizeof(uint4) * n, hipMemcpyDeviceToHost));
  }
  if (pos || flags || objs) {
    for (int64_t i = 0; i < n; ++i) {
      Env e;
      unpack_st4(st[(size_t)i], e);
      if (pos) pos[2 * i] = e.px, pos[2 * i + 1] = e.py;
      if (flags) flags[i] = e.f;
      if (objs) objs[4 * i] = e.kx, objs[4 * i + 1] = e.ky, objs[4 * i + 2] = e.gx, objs[4 * i + 3] = e.gy;
    }
  }
  if (ang) HIP_TRY(hipMemcpy(ang, h->S.ang, sizeof(double2) * n, hipMemcpyDeviceToHost));
  if (ep) {  // (return, start step) -> (return, length): the steps since the start
    HIP_TRY(hipMemcpy(ep, h->S.ep, sizeof(int2) * n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) ep[2 * i + 1] = (int32_t)(h->tstep - (uint32_t)ep[2 * i + 1]);
  }
  if (mt_pos) {
    // CPython's index into the generation holding the position
    for (int64_t i = 0; i < n; ++i) {
      Env e;
      unpack_st4(st[(size_t)i], e);
      mt_pos[i] = (e.mti & MT_POS_MASK) % MT_N;
    }
  }
  if (mt) {
    // the generations, gathered on the device into a bounded staging buffer (<= 64 Ki envs,
    // 160 MB) and copied out in one transfer per chunk
    const int64_t chunk = n < (1 << 16) ? n : (1 << 16);
    DevBuf<uint32_t> stage;
    TG_TRY(stage.alloc(MT_N * (size_t)chunk, "tg_read_state's staging buffer"));
    for (int64_t first = 0; first < n; first += chunk) {
      const int64_t cnt = n - first < chunk ? n - first : chunk;
      const int64_t threads = cnt * (MT_N / 4);
      hipLaunchKernelGGL(k_gather_mt, dim3((unsigned)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK),
                         0, 0, h->S, first, cnt, stage.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(mt + first * MT_N, stage.get(), sizeof(uint32_t) * MT_N * (size_t)cnt,
                        hipMemcpyDeviceToHost));
    }
  }
  return TG_OK;
}

int tg_write_state(tg_batch* h, const int32_t* pos, const uint32_t* flags, const int32_t* objs,
                   const double* ang, const uint32_t* mt, const uint32_t* mt_pos,
                   const int32_t* ep) {
  BIND(h);
  if (!pos || !flags || !objs || !ang || !mt || !mt_pos)
    return fail(TG_E_INVAL, "tg_write_state: pos, flags, objs, ang, mt and mt_pos are required");
  const int64_t n = h->n;
  std::vector<uint4> st((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t p = mt_pos[i];
    if (p > (uint32_t)MT_N || (p & 1u))
      return fail(TG_E_INVAL, "tg_write_state: env %lld: mt_pos %u (must be even, <= 624: "
                  "random() consumes words in pairs)", (long long)i, p);
    for (int k = 0; k < 2; ++k)
      if (pos[2 * i + k] < -32768 || pos[2 * i + k] > 32767)
        return fail(TG_E_INVAL, "tg_write_state: env %lld: position out of range", (long long)i);
    for (int k = 0; k < 4; ++k)
      if (objs[4 * i + k] < -128 || objs[4 * i + k] > 127)
        return fail(TG_E_INVAL, "tg_write_state: env %lld: object cell out of range", (long long)i);
    Env e{};
    e.px = pos[2 * i], e.py = pos[2 * i + 1];
    e.f = flags[i];
    e.kx = objs[4 * i], e.ky = objs[4 * i + 1], e.gx = objs[4 * i + 2], e.gy = objs[4 * i + 3];
    // the given generation goes to the ring's first slot, its successors to the others
    // (fresh); index 624 is the start of the successor (CPython twists before its next draw)
    e.mti = p;
    st[(size_t)i] = pack(e);
  }
  HIP_TRY(hipDeviceSynchronize());
  // validated: the pending refill lists name the old states' halves, and every ring is rebuilt
  h->main.rpend = 0;
  for (auto& c : h->grp) c.rpend = 0;
  HIP_TRY(hipMemset(h->main.regen_ctr.get(), 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
  for (auto& c : h->grp) HIP_TRY(hipMemset(c.regen_ctr.get(), 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
  HIP_TRY(hipMemcpy(h->S.st4, st.data(), sizeof(uint4) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->S.ang, ang, sizeof(double2) * n, hipMemcpyHostToDevice));
  {  // (return, length) -> (return, start step)
    std::vector<int2> e2((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      e2[(size_t)i] = ep ? make_int2(ep[2 * i], (int32_t)(h->tstep - (uint32_t)ep[2 * i + 1]))
                         : make_int2(0, (int32_t)h->tstep);
    HIP_TRY(hipMemcpy(h->S.ep, e2.data(), sizeof(int2) * n, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy2D(h->S.mt, sizeof(uint32_t) * MT_STORE, mt, sizeof(uint32_t) * MT_N,
                      sizeof(uint32_t) * MT_N, (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gen_codes, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n);
  hipLaunchKernelGGL(k_gen_twist, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n, 0u, 1,
                     2 * MT_HALF_GENS - 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return TG_OK;
}

// ---- snapshots ---------------------------------------------------------------------------------
int tg_snap_create(tg_batch* h, int64_t slots, tg_snap** out) {
  BIND(h);
  if (!out || slots <= 0) return fail(TG_E_INVAL, "tg_snap_create: slots %lld, or a null output", (long long)slots);
  *out = nullptr;
  auto s = std::make_unique<tg_snap>();
  s->owner = h;
  s->slots = slots;
  TG_TRY(s->st4.alloc((size_t)slots, "snapshot states"));
  TG_TRY(s->ang.alloc((size_t)slots, "snapshot angles"));
  TG_TRY(s->ep.alloc((size_t)slots, "snapshot episodes"));
  TG_TRY(s->mt.alloc(MT_N * (size_t)slots, "snapshot generations"));
  HIP_TRY(hipMemset(s->st4.get(), 0, sizeof(uint4) * (size_t)slots));
  HIP_TRY(hipMemset(s->ang.get(), 0, sizeof(double2) * (size_t)slots));
  HIP_TRY(hipMemset(s->ep.get(), 0, sizeof(int2) * (size_t)slots));
  HIP_TRY(hipMemset(s->mt.get(), 0, sizeof(uint32_t) * MT_N * (size_t)slots));
  HIP_TRY(hipDeviceSynchronize());
  *out = s.get();
  h->snaps.push_back(std::move(s));
  return TG_OK;
}

void tg_snap_destroy(tg_snap* s) {
  if (!s || !s->owner) return;
  tg_batch* const h = s->owner;
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != h->device) (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();  // no queued save or load runs against a freed slot
  for (auto it = h->snaps.begin(); it != h->snaps.end(); ++it)
    if (it->get() == s) {
      h->snaps.erase(it);  // its buffers: by their owners
      return;
    }
}

int64_t tg_snap_slots(const tg_snap* s) { return s ? s->slots : 0; }

namespace {
Snap snap_view(const tg_snap* s) { return Snap{s->st4.get(), s->ang.get(), s->ep.get(), s->mt.get()}; }
int snap_args(const char* who, const tg_batch* h, const tg_snap* s, const int64_t* envs,
              const int64_t* slots, int64_t count) {
  if (!s || !envs || !slots) return fail(TG_E_INVAL, "%s: a null snapshot, envs or slots", who);
  if (s->owner != h) return fail(TG_E_INVAL, "%s: the snapshot belongs to another handle", who);
  if (count < 0) return fail(TG_E_INVAL, "%s: count %lld < 0", who, (long long)count);
  if (count > (int64_t)1 << 31)  // (the launches' grids)
    return fail(TG_E_INVAL, "%s: count %lld > 2^31", who, (long long)count);
  return TG_OK;
}
int snap_range(const char* who, const tg_snap* s, int64_t first, int64_t count) {
  if (!s) return fail(TG_E_INVAL, "%s: null snapshot", who);
  if (first < 0 || count < 0 || first > s->slots || count > s->slots - first)
    return fail(TG_E_INVAL, "%s: slots [%lld, +%lld) of %lld", who, (long long)first, (long long)count,
                (long long)s->slots);
  return TG_OK;
}
}  // namespace

int tg_snap_save(tg_batch* h, tg_snap* s, const int64_t* envs, const int64_t* slots, int64_t count,
                 void* stream) {
  BIND(h);
  TG_TRY(snap_args("tg_snap_save", h, s, envs, slots, count));
  if (count == 0) return TG_OK;
  const int64_t threads = count * SNAP_Q;
  hipLaunchKernelGGL(k_snap_save, dim3((unsigned)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                     (hipStream_t)stream, h->S, h->n, snap_view(s), s->slots, envs, slots, count,
                     h->tstep, h->err.get());
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_snap_load(tg_batch* h, const tg_snap* s, const int64_t* slots, const int64_t* envs,
                 const uint64_t* seeds, int64_t count, void* stream) {
  BIND(h);
  TG_TRY(snap_args("tg_snap_load", h, s, envs, slots, count));
  if (count == 0) return TG_OK;
  constexpr int WAVES = BLOCK / 64;  // one wavefront per entry
  const dim3 grid((unsigned)((count + WAVES - 1) / WAVES));
  hipStream_t st = (hipStream_t)stream;
  if (seeds) {
    hipLaunchKernelGGL(k_snap_seed, dim3(grid_for(count)), dim3(BLOCK), 0, st, h->S, h->n, s->slots,
                       envs, slots, seeds, count, h->genrand.get());
    hipLaunchKernelGGL(k_snap_load<true>, grid, dim3(BLOCK), 0, st, h->S, h->n, snap_view(s), s->slots,
                       slots, envs, count, h->tstep, h->err.get());
  } else {
    hipLaunchKernelGGL(k_snap_load<false>, grid, dim3(BLOCK), 0, st, h->S, h->n, snap_view(s), s->slots,
                       slots, envs, count, h->tstep, h->err.get());
  }
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_snap_read(tg_snap* s, int64_t first, int64_t count, int32_t* pos, uint32_t* flags,
                 int32_t* objs, double* ang, uint32_t* mt, uint32_t* mt_pos, int32_t* ep) {
  TG_TRY(snap_range("tg_snap_read", s, first, count));
  BIND(s->owner);
  HIP_TRY(hipDeviceSynchronize());
  if (count == 0) return TG_OK;
  if (pos || flags || objs || mt_pos) {
    std::vector<uint4> st((size_t)count);
    HIP_TRY(hipMemcpy(st.data(), s->st4.get() + first, sizeof(uint4) * count, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; ++i) {
      Env e;
      unpack_st4(st[(size_t)i], e);
      if (pos) pos[2 * i] = e.px, pos[2 * i + 1] = e.py;
      if (flags) flags[i] = e.f;
      if (objs) objs[4 * i] = e.kx, objs[4 * i + 1] = e.ky, objs[4 * i + 2] = e.gx, objs[4 * i + 3] = e.gy;
      if (mt_pos) mt_pos[i] = e.mti;
    }
  }
  if (ang) HIP_TRY(hipMemcpy(ang, s->ang.get() + first, sizeof(double2) * count, hipMemcpyDeviceToHost));
  if (ep) HIP_TRY(hipMemcpy(ep, s->ep.get() + first, sizeof(int2) * count, hipMemcpyDeviceToHost));
  if (mt)
    HIP_TRY(hipMemcpy(mt, s->mt.get() + first * MT_N, sizeof(uint32_t) * MT_N * (size_t)count,
                      hipMemcpyDeviceToHost));
  return TG_OK;
}

int tg_snap_write(tg_snap* s, int64_t first, int64_t count, const int32_t* pos, const uint32_t* flags,
                  const int32_t* objs, const double* ang, const uint32_t* mt, const uint32_t* mt_pos,
                  const int32_t* ep) {
  TG_TRY(snap_range("tg_snap_write", s, first, count));
  BIND(s->owner);
  if (!pos || !flags || !objs || !ang || !mt || !mt_pos)
    return fail(TG_E_INVAL, "tg_snap_write: pos, flags, objs, ang, mt and mt_pos are required");
  std::vector<uint4> st((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    const uint32_t p = mt_pos[i];
    if (p > (uint32_t)MT_N || (p & 1u))
      return fail(TG_E_INVAL, "tg_snap_write: record %lld: mt_pos %u (must be even, <= 624: "
                  "random() consumes words in pairs)", (long long)i, p);
    for (int k = 0; k < 2; ++k)
      if (pos[2 * i + k] < -32768 || pos[2 * i + k] > 32767)
        return fail(TG_E_INVAL, "tg_snap_write: record %lld: position out of range", (long long)i);
    for (int k = 0; k < 4; ++k)
      if (objs[4 * i + k] < -128 || objs[4 * i + k] > 127)
        return fail(TG_E_INVAL, "tg_snap_write: record %lld: object cell out of range", (long long)i);
    Env e{};
    e.px = pos[2 * i], e.py = pos[2 * i + 1];
    e.f = flags[i];
    e.kx = objs[4 * i], e.ky = objs[4 * i + 1], e.gx = objs[4 * i + 2], e.gy = objs[4 * i + 3];
    e.mti = p;  // stored as given: tg_snap_load gives 624 tg_write_state's meaning
    st[(size_t)i] = pack(e);
  }
  HIP_TRY(hipDeviceSynchronize());
  if (count == 0) return TG_OK;
  HIP_TRY(hipMemcpy(s->st4.get() + first, st.data(), sizeof(uint4) * count, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->ang.get() + first, ang, sizeof(double2) * count, hipMemcpyHostToDevice));
  if (ep) HIP_TRY(hipMemcpy(s->ep.get() + first, ep, sizeof(int2) * count, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemset(s->ep.get() + first, 0, sizeof(int2) * count));
  HIP_TRY(hipMemcpy(s->mt.get() + first * MT_N, mt, sizeof(uint32_t) * MT_N * (size_t)count,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return TG_OK;
}

// ---- diagnostics and measurement -------------------------------------------------------------
int tg_errors(tg_batch* h, uint32_t* out, void* stream) {
  BIND(h);
  if (!out) return fail(TG_E_INVAL, "tg_errors: null output");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_errors, dim3(grid_for(h->n)), dim3(BLOCK), 0, st, h->S.st4, h->n, h->err.get());
  HIP_TRY(hipGetLastError());
  uint32_t v = 0;
  HIP_TRY(hipMemcpyAsync(&v, h->err.get(), sizeof v, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out = v;
  return TG_OK;
}

int tg_set_timing(tg_batch* h, int every) {
  BIND(h);
  if (every < 0) return fail(TG_E_INVAL, "tg_set_timing: every %d < 0", every);
  HIP_TRY(hipDeviceSynchronize());
  TG_TRY(flush_timing(h->tm));  // records of the previous setting are kept in the sums
  if (every && !h->tm.kst) TG_TRY(kst_reset(h->tm));
  h->tm.every = every;
  h->tm.calls = 0;
  return TG_OK;
}

int tg_get_stats(tg_batch* h, tg_stats* out) {
  BIND(h);
  if (!out) return fail(TG_E_INVAL, "tg_get_stats: null output");
  HIP_TRY(hipDeviceSynchronize());
  TG_TRY(flush_timing(h->tm));
  unsigned long long s[ST_COUNT] = {};
  std::vector<StepCtx*> ctxs{&h->main};
  for (auto& c : h->grp) ctxs.push_back(&c);
  for (StepCtx* c : ctxs) {
    const size_t nb = (size_t)stat_slots(c->n);
    std::vector<unsigned long long> part(nb * ST_COUNT);
    HIP_TRY(hipMemcpy(part.data(), c->stats.get(), sizeof(unsigned long long) * part.size(),
                      hipMemcpyDeviceToHost));
    for (size_t b = 0; b < nb; ++b)
      for (int k = 0; k < ST_COUNT; ++k) s[k] += part[b * ST_COUNT + k];
  }
  out->steps = (int64_t)s[ST_STEPS];
  out->valid_steps = (int64_t)s[ST_VALID];
  out->ticks = (int64_t)s[ST_TICKS];
  out->draws = (int64_t)s[ST_DRAWS];
  out->episodes = (int64_t)s[ST_EPISODES];
  out->episodes_dropped = (int64_t)s[ST_EP_OVERFLOW];
  out->launches = out->steps / (h->n ? h->n : 1);
  const Timing::Sums& t = h->tm.sums;
  out->kernel_ms = t.kernel_ms;
  out->regens = (int64_t)s[ST_REGENS] * MT_HALF_GENS;  // halves -> generations
  out->regens_quiet = (int64_t)s[ST_RQUIET] * MT_HALF_GENS;
  out->wave_ticks = (int64_t)s[ST_WTICKS];
  out->timed_launches = t.timed_launches;
  out->run_ms = t.run_ms;
  out->regen_ms = t.regen_ms;
  out->regen_timed = t.regen_timed;
  out->regen_launches = t.regen_launches;
  out->classify_ms = t.classify_ms;
  out->episodes_truncated = (int64_t)s[ST_TRUNC];
  return TG_OK;
}

int tg_stats_reset(tg_batch* h) {
  BIND(h);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(h->main.stats.get(), 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(h->n)));
  for (auto& c : h->grp)
    HIP_TRY(hipMemset(c.stats.get(), 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(c.n)));
  if (h->tm.kst) TG_TRY(kst_reset(h->tm));  // drops the unflushed records
  h->tm.sums = {};
  return TG_OK;
}

int64_t tg_live_resources(void) { return tg::g_live.load(std::memory_order_relaxed); }

int tg_probe_dispatch(int32_t kernels, int32_t blocks, void* stream) {
  if (kernels < 0 || blocks < 1) return fail(TG_E_INVAL, "tg_probe_dispatch: bad arguments");
  for (int32_t k = 0; k < kernels; ++k)
    hipLaunchKernelGGL(k_null, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

int tg_mt_layout(int32_t* ring_words, int32_t* stored_words, int32_t* code_bytes) {
  if (ring_words) *ring_words = MT_WORDS;
  if (stored_words) *stored_words = MT_STORE;
  if (code_bytes) *code_bytes = MT_CODES;
  return TG_OK;
}

int tg_kernel_info(tg_batch* h, int kernel, int32_t* blocks_per_cu, int32_t* vgprs, int32_t* sgprs,
                   int32_t* lds_bytes) {
  BIND(h);
  const void* k = kernel == TG_KERNEL_CLASSIFY ? reinterpret_cast<const void*>(k_classify<true, false>)
                  : kernel == TG_KERNEL_RUN    ? reinterpret_cast<const void*>(k_run<true, false>)
                  : kernel == TG_KERNEL_REGEN  ? reinterpret_cast<const void*>(k_regen)
                                               : nullptr;
  if (!k) return fail(TG_E_INVAL, "tg_kernel_info: unknown kernel %d", kernel);
  hipFuncAttributes fa;
  HIP_TRY(hipFuncGetAttributes(&fa, k));
  int nb = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, kernel == TG_KERNEL_RUN ? RUN_BLOCK : BLOCK,
                                                       0));
  if (blocks_per_cu) *blocks_per_cu = nb;
  if (vgprs) *vgprs = fa.numRegs;
  if (sgprs) *sgprs = -1;  // not reported by hipFuncGetAttributes
  if (lds_bytes) *lds_bytes = (int32_t)fa.sharedSizeBytes;
  return TG_OK;
}

int tg_predicate_table(tg_batch* h, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                       uint32_t door_bits, uint8_t* out, void* stream) {
  BIND(h);
  if (!out || x1 <= x0 || y1 <= y0 || x0 < -4096 || x1 > 32000 || y0 < -4096 || y1 > 32000)
    return fail(TG_E_INVAL, "tg_predicate_table: bad box or null output");
  const int64_t cells = (int64_t)(x1 - x0) * (y1 - y0);
  hipLaunchKernelGGL(k_predicates, dim3((unsigned)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                     (hipStream_t)stream, h->L, h->grid.get(), x0, x1, y0, y1, door_bits, out);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

#ifdef TG_DIAG_STAMPS
int tg_diag_stamps(unsigned long long* out, int n_waves) {
  if (n_waves > NSTAMP_WAVES) n_waves = NSTAMP_WAVES;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * NSTAMP * n_waves));
  return TG_OK;
}
#endif

}  // extern "C"
