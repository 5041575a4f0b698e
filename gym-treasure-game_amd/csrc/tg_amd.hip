// tg_amd.hip — MI355X (gfx950) batched Treasure Game: the host code and the C ABI of
// include/tg_amd.h.  The kernels it launches are in the headers it includes: tg_dev.h (the device
// layer shared with k_flow's unit, tg_flow.hip; the state layout is described there),
// tg_kernels.h (the batch kernels), tg_py1.h (the N = 1 path) and tg_flow.h (TG_MODE_FLOW's
// types; k_flow itself is instantiated by tg_flow.hip and reached through tg::flow_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tg_amd.h"
#include "tg_dev.h"
#include "tg_flow.h"
#include "tg_kernels.h"
#include "tg_py1.h"

namespace tg {
thread_local std::string g_err;
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

// hipMalloc, or leave the calling function with TG_E_NOMEM
#define ALLOC(ptr, bytes)                               \
  if (hipMalloc((void**)&(ptr), (bytes)) != hipSuccess) \
    return fail(TG_E_NOMEM, "hipMalloc %zu B for " #ptr, (size_t)(bytes))

// ---- timing (tg_set_timing) ------------------------------------------------------------------
// The kernels of a sampled step launch (and every k_regen launch while timing is on) fold their
// in-kernel span stamps into the launch's record (kst_end): no event or other packet goes on the
// stream.  Records: KST_MAX step samples (two kernels each) and KST_MAX k_regen launches,
// KST_SLOTS slots per kernel.
constexpr int KST_MAX = 512;
constexpr int64_t KST_KSLOTS = (int64_t)KST_MAX * 3 * KST_SLOTS;  // slots of all records
unsigned long long* kst_step(tg_batch* h, int k, int kernel) {
  return h->kst + ((size_t)k * 2 + kernel) * KST_STRIDE * KST_SLOTS;
}
unsigned long long* kst_regen(tg_batch* h, int k) {
  return h->kst + ((size_t)KST_MAX * 2 + k) * KST_STRIDE * KST_SLOTS;
}
int kst_reset(tg_batch* h) {  // every record to (no start, no end)
  if (!h->kst && hipMalloc((void**)&h->kst, sizeof(unsigned long long) * KST_STRIDE * KST_KSLOTS) !=
                     hipSuccess)
    return fail(TG_E_NOMEM, "timing records");
  hipLaunchKernelGGL(k_kst_init, dim3((unsigned)((KST_KSLOTS + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0,
                     h->kst, KST_KSLOTS);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  h->kst_steps = 0;
  h->kst_regens = 0;
  h->kst_k.clear();
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
int flush_timing(tg_batch* h) {
  if (!h->kst_steps && !h->kst_regens) return TG_OK;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<unsigned long long> rec((size_t)KST_STRIDE * KST_KSLOTS);
  HIP_TRY(hipMemcpy(rec.data(), h->kst, sizeof(unsigned long long) * rec.size(), hipMemcpyDeviceToHost));
  const size_t kr = (size_t)KST_STRIDE * KST_SLOTS;  // u64 per kernel record
  for (int k = 0; k < h->kst_steps; ++k) {
    const double c = kst_span_ms(rec.data() + (k * 2 + 0) * kr), r = kst_span_ms(rec.data() + (k * 2 + 1) * kr);
    h->classify_ms_done += c;
    h->run_ms_done += r;
    h->kernel_ms_done += c + r;
    h->timed_launches += k < (int)h->kst_k.size() ? h->kst_k[(size_t)k] : 1;  // k_flow: K steps
  }
  for (int k = 0; k < h->kst_regens; ++k) {
    h->regen_ms_done += kst_span_ms(rec.data() + ((size_t)KST_MAX * 2 + k) * kr);
    ++h->regen_timed;
  }
  return kst_reset(h);
}
// a step launch covering k steps: if it is sampled, ks0 / ks1 are its kernels' records (else null)
int timing_begin(tg_batch* h, unsigned long long*& ks0, unsigned long long*& ks1, int k = 1) {
  ks0 = ks1 = nullptr;
  if (!h->timing_every || (h->timing_calls++ % (uint64_t)h->timing_every) != 0) return TG_OK;
  if (h->kst_steps >= KST_MAX)
    if (const int rc = flush_timing(h)) return rc;
  ks0 = kst_step(h, h->kst_steps, 0);
  ks1 = kst_step(h, h->kst_steps, 1);
  ++h->kst_steps;
  h->kst_k.push_back(k);
  return TG_OK;
}

// ---- steppers (StepCtx) ----------------------------------------------------------------------
// a stepper's buffers for envs [off, off + n)
int alloc_ctx(StepCtx& c, int64_t off, int64_t n) {
  c.off = off;
  c.n = n;
  ALLOC(c.stats, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(n));
  // a worklist shard holds the envs of every WSHARDS-th workgroup; a refill list those of every
  // SHARDS-th, REGEN_STEPS steps of them
  c.shard_cap = (int64_t)((grid_for(n) + WSHARDS - 1) / WSHARDS) * BLOCK;
  ALLOC(c.wl, sizeof(int32_t) * NSEG * (size_t)c.shard_cap);
  ALLOC(c.wst4, sizeof(uint4) * NSEG * (size_t)c.shard_cap);
  ALLOC(c.wang, sizeof(double2) * NSEG * (size_t)c.shard_cap);
  ALLOC(c.wep, sizeof(int2) * NSEG * (size_t)c.shard_cap);
  ALLOC(c.wctr, sizeof(int32_t) * 2 * NCTR * CTR_STRIDE);
  // a shard's list holds at most its workgroups' envs per pending step
  c.rcap = (int64_t)((grid_for(n) + SHARDS - 1) / SHARDS) * BLOCK * REGEN_STEPS;
  ALLOC(c.refill, sizeof(uint32_t) * SHARDS * (size_t)c.rcap);
  ALLOC(c.regen_ctr, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE);
  // a quiet list holds one step's entries: drained by the k_run of the step that appended them
  c.qcap = (int64_t)((grid_for(n) + SHARDS - 1) / SHARDS) * BLOCK;
  ALLOC(c.quiet, sizeof(uint32_t) * SHARDS * (size_t)c.qcap);
  HIP_TRY(hipMemset(c.stats, 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(n)));
  HIP_TRY(hipMemset(c.wctr, 0, sizeof(int32_t) * 2 * NCTR * CTR_STRIDE));
  HIP_TRY(hipMemset(c.regen_ctr, 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
  return TG_OK;
}
void free_ctx(StepCtx& c) {
  void* bufs[] = {c.stats, c.wl, c.wst4, c.wang, c.wep, c.wctr, c.refill, c.regen_ctr, c.quiet};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c.ev) (void)hipEventDestroy(c.ev);
  if (c.st) (void)hipStreamDestroy(c.st);
  c = StepCtx{};
}
// a stepper's envs as a Soa view (envs [off, off + n) of the handle)
Soa soa_of(const tg_batch* h, const StepCtx& c) {
  return Soa{h->S.st4 + c.off, h->S.ang + c.off, h->S.ep + c.off, h->S.mt + c.off * (int64_t)MT_STORE,
             h->S.mc + c.off * (int64_t)MT_CODES};
}
// k_regen over the stepper's pending refill lists (its span recorded when timing is on: the
// handle's own stepper only)
int launch_regen(tg_batch* h, StepCtx& c, hipStream_t st) {
  if (!c.rpend) return TG_OK;
  unsigned long long* ks = nullptr;
  if (h->timing_every && &c == &h->main) {
    if (h->kst_regens >= KST_MAX) {
      const int rc = flush_timing(h);
      if (rc) return rc;
    }
    ks = kst_regen(h, h->kst_regens++);
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
  int32_t* const cur = c.regen_ctr + c.regen_parity * RCTR_N * CTR_STRIDE;
  int32_t* const nxt = c.regen_ctr + (c.regen_parity ^ 1) * RCTR_N * CTR_STRIDE;
  c.regen_parity ^= 1;
  hipLaunchKernelGGL(k_regen, dim3((unsigned)grid), dim3(BLOCK), 0, st, soa_of(h, c), c.refill,
                     c.rcap, cur, nxt, c.stats, stat_slots(c.n), ks);
  HIP_TRY(hipGetLastError());
  c.rpend = 0;
  ++h->regen_launches;
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
// first group)
int launch_step(tg_batch* h, StepCtx& c, const StepIO& io_in, bool ar, hipStream_t st,
                uint32_t tstep, hipEvent_t mid = nullptr) {
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
    if (const int rc = timing_begin(h, ks0, ks1)) return rc;
  const EpQueue q{h->eps, h->eps_count, h->eps_cap};
  const dim3 grid(grid_for(c.n)), block(BLOCK);
  const Soa S = soa_of(h, c);
  const int64_t g0 = h->g0 + c.off;
  if (h->mode == TG_MODE_DIRECT) {
    const auto kern = step_inst(ar, fo, io.policy,
                                [](auto AR, auto FO, auto POL) { return &k_step<AR, FO, POL>; });
    hipLaunchKernelGGL(kern, grid, block, 0, st, S, c.n, h->L, h->grid, io, q, g0, c.stats, h->err,
                       ks1);
  } else {
    // counters double-buffered by step parity: k_classify zeroes the next step's set (the
    // previous k_run, which read it, has finished), so no memset launch per step
    int32_t* const cur = c.wctr + (c.parity ? NCTR * CTR_STRIDE : 0);
    int32_t* const nxt = c.wctr + (c.parity ? 0 : NCTR * CTR_STRIDE);
    c.parity ^= 1;
    // the refill lists append until k_regen drains them (every REGEN_STEPS steps), counted in
    // the set the next k_regen reads
    const Work w{c.wl,     c.wst4, c.wang, c.wep, cur, nxt, c.refill,
                 c.regen_ctr + (c.regen_parity * RCTR_N + RCTR_LIST) * CTR_STRIDE, c.rcap,
                 c.shard_cap, c.quiet, c.qcap};
    const auto kc = step_inst(ar, fo, io.policy,
                              [](auto AR, auto FO, auto POL) { return &k_classify<AR, FO, POL>; });
    const auto kr = step_inst(ar, fo, -1, [](auto AR, auto FO, auto) { return &k_run<AR, FO>; });
    hipLaunchKernelGGL(kc, grid, block, 0, st, S, c.n, h->L, h->grid, io, q, w, g0, c.stats, h->err,
                       ks0);
    HIP_TRY(hipGetLastError());
    if (mid) HIP_TRY(hipEventRecord(mid, st));  // (the rollouts' stagger between groups)
    hipLaunchKernelGGL(kr, dim3(run_grid_for(c.n) * (BLOCK / RUN_BLOCK)), dim3(RUN_BLOCK), 0, st, S,
                       c.n, h->L, h->grid, io, q, w,
                       g0, c.stats, h->err, ks1);
  }
  HIP_TRY(hipGetLastError());
  if (h->mode != TG_MODE_DIRECT && ++c.rpend == REGEN_STEPS) return launch_regen(h, c, st);
  return TG_OK;
}

// ---- rollouts (tg_rollout, tg_rollout_mlp) ---------------------------------------------------
// what `who` (the entry point's name) checks and prepares: the outputs, and the obs scratch
int rollout_prep(tg_batch* h, const char* who, int32_t steps, bool selector_ok, const double* obs,
                 const int32_t* reward, const uint8_t* valid, const uint8_t* done) {
  if (steps < 0 || !reward || !valid || !done || !selector_ok)
    return fail(TG_E_INVAL, "%s: bad arguments", who);
  if (!obs && !h->obs_scratch)  // the step kernels always write an obs row
    if (hipMalloc((void**)&h->obs_scratch, sizeof(double) * 9 * (size_t)h->n) != hipSuccess)
      return fail(TG_E_NOMEM, "%s: obs scratch", who);
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
  HIP_TRY(hipEventRecord(h->fork, cs));
  for (auto& c : h->grp) HIP_TRY(hipStreamWaitEvent(c.st, h->fork, 0));
  for (int32_t s = 0; s < steps; ++s)
    for (size_t g = 0; g < h->grp.size(); ++g) {
      StepCtx& c = h->grp[g];
      // stagger: group g + 1 starts after group g's first k_classify (half a step apart)
      hipEvent_t mid = (s == 0 && h->stagger && g + 1 < h->grp.size()) ? h->grp[g + 1].ev : nullptr;
      if ((rc = step_of(c, s, c.st, mid))) return rc;
      if (mid) HIP_TRY(hipStreamWaitEvent(h->grp[g + 1].st, mid, 0));
    }
  for (auto& c : h->grp) {
    if ((rc = launch_regen(h, c, c.st))) return rc;
    HIP_TRY(hipEventRecord(c.ev, c.st));
    HIP_TRY(hipStreamWaitEvent(cs, c.ev, 0));
  }
  return TG_OK;
}

// ---- TG_MODE_FLOW (tg_flow.h) ----------------------------------------------------------------
void flow_free(tg_batch* h) {
  auto& F = h->fl;
  void* bufs[] = {F.ctl[0], F.ctl[1], F.q[0], F.q[1], F.fill[0], F.fill[1], F.list, F.outst};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  F = {};
}
// the XCD census (sub-problems) and the work structures, at the first flow rollout
int flow_init(tg_batch* h) {
  auto& F = h->fl;
  if (F.ready) return TG_OK;
  uint32_t* dmask = nullptr;
  if (hipMalloc((void**)&dmask, sizeof(uint32_t)) != hipSuccess) return fail(TG_E_NOMEM, "flow census");
  uint32_t mask = 0;
  hipError_t e = hipMemset(dmask, 0, sizeof(uint32_t));
  if (e == hipSuccess) {
    // several workgroups per CU: every XCD of the device gets some (dispatch is round-robin)
    hipLaunchKernelGGL(k_census, dim3((unsigned)(h->cus * 8)), dim3(64), 0, 0, dmask);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&mask, dmask, sizeof mask, hipMemcpyDeviceToHost);
  (void)hipFree(dmask);
  if (e != hipSuccess) return fail(TG_E_HIP, "flow census: %s", hipGetErrorString(e));
  mask &= 0xFFu;
  F.P = 0;
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
  bool ok = true;
  for (int k = 0; k < 2; ++k)
    ok = ok && hipMalloc((void**)&F.ctl[k], sizeof(int32_t) * nctl) == hipSuccess &&
         hipMalloc((void**)&F.q[k], sizeof(uint32_t) * nq) == hipSuccess &&
         hipMalloc((void**)&F.fill[k], sizeof(int32_t) * nfill) == hipSuccess &&
         hipMemset(F.ctl[k], 0, sizeof(int32_t) * nctl) == hipSuccess &&
         hipMemset(F.q[k], 0xFF, sizeof(uint32_t) * nq) == hipSuccess &&
         hipMemset(F.fill[k], 0, sizeof(int32_t) * nfill) == hipSuccess;
  ok = ok && hipMalloc((void**)&F.list, sizeof(int32_t) * nlist) == hipSuccess &&
       hipMalloc((void**)&F.outst, sizeof(int32_t) * (size_t)C) == hipSuccess;
  if (!ok) {
    flow_free(h);
    return fail(TG_E_NOMEM, "flow work structures (%zu MB of lists)", nlist * 4 >> 20);
  }
  HIP_TRY(hipDeviceSynchronize());
  F.ready = true;
  return TG_OK;
}
// k steps (<= FLOW_MAX_K) of the handle's own stepper in one k_flow launch; outputs at step s0
// of the rollout's [K][N] arrays
int launch_flow(tg_batch* h, int k, const FlowIO& io, bool ar, int pol, hipStream_t st) {
  auto& F = h->fl;
  StepCtx& c = h->main;
  // the MT slack (k_regen every REGEN_STEPS steps): drain first if these steps would overrun it
  if (c.rpend + k > REGEN_STEPS) {
    const int rc = launch_regen(h, c, st);
    if (rc) return rc;
  }
  const void* const kern = tg::flow_kernel(ar, pol);
  int& bpc = F.bpc[ar ? 1 : 0][pol ? 1 : 0];
  if (!bpc) {
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kern, BLOCK, 0));
    if (bpc < 1) bpc = 1;
  }
  unsigned long long *ks0 = nullptr, *ks = nullptr;  // one kernel: the record's second span, as k_run
  if (const int rc = timing_begin(h, ks0, ks, k)) return rc;
  const int p = F.parity;
  F.parity ^= 1;
  Flow f{F.ctl[p], F.q[p], F.fill[p], F.list, F.outst, F.ctl[p ^ 1], F.q[p ^ 1], F.fill[p ^ 1],
         c.refill, c.regen_ctr + (c.regen_parity * RCTR_N + RCTR_LIST) * CTR_STRIDE, c.rcap,
         F.qcap, F.jcap, F.lcap, F.C, F.P, k, F.xmap, h->flow_skip, nullptr, nullptr, nullptr};
#ifdef TG_FLOW_DBG
  if (const int rc = flow_diag_setup(h, f)) return rc;
#endif
  const EpQueue q{h->eps, h->eps_count, h->eps_cap};
  if (h->flow_debug)
    fprintf(stderr, "[flow] launching k %d grid %d x %d lcap %lld qcap %lld jcap %lld C %d\n", k, h->cus, bpc,
            (long long)F.lcap, (long long)F.qcap, (long long)F.jcap, F.C);
  {  // k_flow's arguments, in its parameter order and types
    Soa a_s = h->S;
    int64_t a_n = h->n;
    Level a_l = h->L;
    const uint32_t* a_grid = h->grid;
    FlowIO a_io = io;
    EpQueue a_q = q;
    int64_t a_g0 = h->g0;
    unsigned long long* a_stats = c.stats;
    int a_nstat = stat_slots(h->n);
    uint32_t* a_err = h->err;
    unsigned long long* a_ks = ks;
    void* args[] = {&a_s, &a_n, &a_l, &a_grid, &a_io, &a_q, &f,
                    &a_g0, &a_stats, &a_nstat, &a_err, &a_ks};
    HIP_TRY(hipLaunchKernel(kern, dim3((unsigned)(h->cus * bpc)), dim3(BLOCK), args, 0, st));
  }
  HIP_TRY(hipGetLastError());
  ++F.launches;
  // every sub-problem's chunks finished (no XCD the census saw went without waves)
  hipLaunchKernelGGL(k_flow_check, dim3(1), dim3(64), 0, st, F.ctl[p], F.P, F.C, h->err);
  HIP_TRY(hipGetLastError());
#ifdef TG_FLOW_DBG
  if (const int rc = flow_diag_after(h, f, k, bpc, st)) return rc;
#endif
  if (h->flow_debug) {  // diagnostics: the census and every sub-problem's counters
    HIP_TRY(hipDeviceSynchronize());
    std::vector<int32_t> cw((size_t)F.P * CTL_WORDS);
    HIP_TRY(hipMemcpy(cw.data(), F.ctl[p], sizeof(int32_t) * cw.size(), hipMemcpyDeviceToHost));
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, h->err, sizeof err, hipMemcpyDeviceToHost));
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
  const int hi = h->mlp_hidden == 16 ? 0 : h->mlp_hidden == 32 ? 1 : h->mlp_hidden == 64 ? 2 : 3;
  StepCtx view;
  view.off = off;
  hipLaunchKernelGGL(kern[hi][h->mlp_act], dim3(grid_for(cnt)), dim3(BLOCK), 0, st, soa_of(h, view),
                     cnt, h->L, h->grid, h->mlp_params, h->mlp_masked, mode, a0, h->g0 + off, t,
                     actions + off, logp ? logp + off : nullptr, value ? value + off : nullptr,
                     logits ? logits + off * MLP_OUT : nullptr);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

// ---- N = 1: the calls' buffers, the resident server (k_serve1), k_py1 ------------------------
int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
// pinned, coherent host memory the device writes, and its device-side address (allocated once)
template <class T>
int pinned(T*& host, T*& dev, const char* who, const char* what) {
  if (host) return TG_OK;
  if (hipHostMalloc((void**)&host, sizeof(T), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return fail(TG_E_NOMEM, "%s: pinned %s", who, what);
  HIP_TRY(hipHostGetDevicePointer((void**)&dev, host, 0));
  return TG_OK;
}
// the N = 1 calls' result row
int one_row(tg_batch* h) { return pinned(h->one, h->one_dev, "tg_step1", "result buffer"); }
int row_out(const tg_batch* h, double* obs, int32_t* reward, uint8_t* valid, uint8_t* done) {
  memcpy(obs, h->one->obs, sizeof h->one->obs);
  *reward = h->one->reward;
  *valid = h->one->valid;
  *done = h->one->done;
  return TG_OK;
}
// the Python stream's state (tg_pystate, pinned) and its generations' cache on the device
int py_buffers(tg_batch* h, const char* who) {
  if (const int rc = pinned(h->py, h->py_dev, who, "stream state")) return rc;
  if (!h->pyc) {
    if (hipMalloc((void**)&h->pyc, sizeof(uint32_t) * PY_GENS * MT_N) != hipSuccess)
      return fail(TG_E_NOMEM, "%s: stream cache", who);
    h->py_warm = false;
  }
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
void srv_post_quit(tg_batch* h) {
  SrvBox* const b = h->box;
  b->word = srv_word(SRV_QUIT, 0, false, false, 0);
  __atomic_store_n(&b->seq, ++h->srv_seq, __ATOMIC_RELEASE);
}
struct SrvReaper {
  ~SrvReaper() {
    std::lock_guard<std::mutex> lk(g_srv_mu);
    for (tg_batch* h : g_srv_handles) {
      if (!h->srv_live || hipSetDevice(h->device) != hipSuccess) continue;
      if (hipEventQuery(h->srv_ev) == hipErrorNotReady) srv_post_quit(h);
      const int64_t t0 = now_ns();
      while (hipEventQuery(h->srv_ev) == hipErrorNotReady && now_ns() - t0 < 1000000000ll) {
      }
      h->srv_live = false;
    }
    g_srv_handles.clear();
  }
} g_srv_reaper;

// launch k_serve1 on the server's stream, after the work queued on the caller's stream
int srv_start(tg_batch* h, hipStream_t caller) {
  // every buffer the server may write, whichever call launches it (a server first launched by
  // tg_available_mask1 serves the steps after it too)
  if (const int rc = one_row(h)) return rc;
  if (!h->box) {
    if (const int rc = pinned(h->box, h->box_dev, "tg_step1", "server mailbox")) return rc;
    memset(h->box, 0, sizeof(SrvBox));
    HIP_TRY(hipStreamCreateWithFlags(&h->srv_st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->srv_ev, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->srv_dep, hipEventDisableTiming));
    h->srv_seq = 0;
  }
  // (the stream state is the server's kernel argument; only SRV_*_PY commands touch it)
  if (const int rc = py_buffers(h, "tg_step1")) return rc;
  HIP_TRY(hipEventRecord(h->srv_dep, caller));
  HIP_TRY(hipStreamWaitEvent(h->srv_st, h->srv_dep, 0));
  const EpQueue q{h->eps, h->eps_count, h->eps_cap};
  if (h->srv_stage < 0) {  // the level's tables into the server's LDS, those that fit
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
    if (dyn > 65536 &&
        hipFuncSetAttribute((const void*)k_serve1, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)dyn) != hipSuccess) {
      (void)hipGetLastError();
      stage = 0u;
      dyn = 0;
    }
    h->srv_stage = (int)stage;
    h->srv_dyn = dyn;
  }
  if (!h->box_dev || !h->py_dev || !h->pyc || !h->one_dev || !h->S.st4 || !h->S.ang || !h->S.ep ||
      !h->S.mt || !h->S.mc || !h->grid || !h->main.stats || !h->err)
    return fail(TG_E_HIP, "k_serve1: a buffer it writes is not allocated");
  hipLaunchKernelGGL(k_serve1, dim3(1), dim3(64), h->srv_dyn, h->srv_st, h->S, h->L, h->grid,
                     h->box_dev, h->py_dev, h->pyc, h->one_dev, q, h->g0, h->srv_idle,
                     (int)h->srv_trace, (uint32_t)h->srv_stage, h->main.stats, h->err);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(h->srv_ev, h->srv_st));
  h->srv_live = true;
  srv_register(h, true);
  h->srv_t_last = now_ns();
  ++h->srv_launches;
  return TG_OK;
}

// post a command and spin on its answer; a server that left (idle) before it saw the command is
// relaunched, and the new one serves it (it starts from the mailbox's done)
int srv_call(tg_batch* h, const SrvBox& c, hipStream_t caller) {
  // a server idle for more than half its limit (host clock, which starts after the server's)
  // may have left: ask its event before posting
  const int64_t t0 = now_ns();
  if (!h->srv_live ||
      (t0 - h->srv_t_last > (int64_t)h->srv_idle * 5 && hipEventQuery(h->srv_ev) == hipSuccess)) {
    if (const int rc = srv_start(h, caller)) return rc;
  }
  SrvBox* const b = h->box;
  const uint32_t seq = ++h->srv_seq;
  b->word = c.word;
  b->tstep = c.tstep;
  b->gauss_bits = c.gauss_bits;
  const int64_t tp = h->srv_trace ? now_ns() : 0;
  __atomic_store_n(&b->seq, seq, __ATOMIC_RELEASE);
  ++h->srv_calls;
  for (uint64_t it = 1;; ++it) {
    if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) {
      h->srv_t_last = now_ns();
      if (h->srv_trace) {
        const double g = 10.0 * (double)(b->t_end - b->t_seen), k = (double)b->ticks;
        h->srv_post_ns += (double)(tp - t0);
        h->srv_rt_ns += (double)(h->srv_t_last - tp);
        h->srv_gpu_ns += g;
        h->srv_fit[0] += k;
        h->srv_fit[1] += k * k;
        h->srv_fit[2] += g * k;
        if (b->phase[0]) {  // py_call's phases: pickup -> option start -> end -> observe ->
          const uint64_t t[7] = {b->t_seen, b->phase[0], b->phase[1], b->phase[2], b->phase[3],
                                 b->phase[4], b->t_end};  // barrier -> its return -> answer
          for (int j = 0; j < 6; ++j) h->srv_phase[j] += 10.0 * (double)(t[j + 1] - t[j]);
          ++h->srv_phase_n;
        }
      }
      return TG_OK;
    }
    __builtin_ia32_pause();
    if ((it & 4095) == 0) {
      const hipError_t e = hipEventQuery(h->srv_ev);
      if (e == hipSuccess) {  // the server left: a new one serves the command
        if (__atomic_load_n(&b->done, __ATOMIC_ACQUIRE) == seq) continue;
        if (const int rc = srv_start(h, caller)) return rc;
      } else if (e != hipErrorNotReady) {
        h->srv_live = false;
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
  if (const int rc = one_row(h)) return rc;
  if (const int rc = py_buffers(h, "tg_*1_py")) return rc;
  // the device's cached generations serve the call iff the caller's state is the one the last
  // call returned (no other draws on the stream since: the user's own, another env's)
  const bool warm = h->py_warm && *index == h->py_last.index &&
                    (!has_gauss || (*has_gauss == h->py_last.has_gauss &&
                                    memcmp(gauss_next, &h->py_last.gauss_next, sizeof(double)) == 0)) &&
                    memcmp(words, h->py_last.mt, sizeof h->py_last.mt) == 0;
  if (!warm) {
    memcpy(h->py->mt, words, sizeof h->py->mt);
    h->py->index = *index;
  }
  if (has_gauss) {
    h->py->has_gauss = *has_gauss;
    h->py->gauss_next = *gauss_next;
  }
  const uint32_t q0 = *index;
  const int hg = has_gauss ? (int)*has_gauss : 0;
  const double gn = has_gauss ? *gauss_next : 0.0;
  // a step's tstep is its index; a reset's, the next step's (the new episode's start)
  const uint32_t tstep = RESET ? h->tstep : h->tstep++;
  h->py_warm = false;  // until the call has returned
  if (h->serve) {
    SrvBox c{};
    c.word = srv_word(RESET ? SRV_RESET_PY : SRV_STEP_PY, action, warm, hg != 0, q0);
    c.tstep = tstep;
    memcpy(&c.gauss_bits, &gn, sizeof c.gauss_bits);
    if (const int rc = srv_call(h, c, stream)) return rc;
  } else {
    hipLaunchKernelGGL(k_py1<RESET>, dim3(1), dim3(64), 0, stream, h->S, h->L, h->grid, (int)action,
                       h->py_dev, warm ? h->pyc : nullptr, h->pyc, q0, hg, gn, h->one_dev, tstep,
                       h->main.stats, h->err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
  }
  memcpy(words, h->py->mt, sizeof h->py->mt);
  *index = h->py->index;
  memcpy(h->py_last.mt, words, sizeof h->py_last.mt);
  h->py_last.index = *index;
  if (has_gauss) {
    *has_gauss = h->py->has_gauss;
    *gauss_next = h->py->gauss_next;
    h->py_last.has_gauss = *has_gauss;
    h->py_last.gauss_next = *gauss_next;
  }
  h->py_warm = true;
  return TG_OK;
}

}  // namespace

namespace tg {
int srv_stop(tg_batch* h) {
  if (!h->srv_live) return TG_OK;
  h->srv_live = false;
  srv_register(h, false);
  if (hipEventQuery(h->srv_ev) != hipSuccess) srv_post_quit(h);
  HIP_TRY(hipEventSynchronize(h->srv_ev));
  // gone: a QUIT it left (idle) without reading is void, not a command for the next server
  h->box->done = h->box->seq;
  return TG_OK;
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

  tg_batch* h = new tg_batch();
  h->device = device;
  h->cus = prop.multiProcessorCount;
  h->n = n;
  h->g0 = global_offset;
  h->seed0 = seed_base;
  h->domain = dom;
  h->flow_debug = getenv("TG_FLOW_DEBUG") != nullptr;
  if (const char* sp = getenv("TG_FLOW_SKIP_PART")) h->flow_skip = atoi(sp);
  if (const char* sv = getenv("TG_SERVE")) h->serve = atoi(sv) != 0;
  h->srv_trace = getenv("TG_SERVE_TRACE") != nullptr;
  // the server's idle limit: 500 us by default (a stream it shares a hardware queue with waits
  // at most this long behind it)
  const char* si = getenv("TG_SERVE_IDLE_US");
  h->srv_idle = 100u * (uint32_t)std::min(std::max(si ? atoi(si) : 500, 1), 1000000);
  // completed-episode queue: drained by tg_episodes; records beyond it are counted as dropped
  const int64_t cap = 4 * n > (1 << 16) ? 4 * n : (1 << 16);
  h->eps_cap = (int32_t)(cap < (1 << 28) ? cap : (1 << 28));
  auto cleanup = [&](int code) {
    tg_destroy(h);
    return code;
  };
  uint32_t gen[MT_N];
  gen[0] = 19650218u;  // init_genrand(19650218) — the common prefix of init_by_array
  for (int i = 1; i < MT_N; ++i) gen[i] = 1812433253u * (gen[i - 1] ^ (gen[i - 1] >> 30)) + (uint32_t)i;
  grid.resize((grid.size() + 3) & ~(size_t)3, 0);
  const std::vector<uint32_t> gotab = build_gotab(L, grid);
  const std::vector<uint32_t> masks = build_masks(L, grid);
  const std::vector<double> obs_q = build_obs_q(L);
  auto alloc = [&]() -> int {
    ALLOC(h->grid, grid.size());
    ALLOC(h->genrand, sizeof gen);
    ALLOC(h->gotab, sizeof(uint32_t) * gotab.size());
    if (!masks.empty()) ALLOC(h->masks, sizeof(uint32_t) * masks.size());
    ALLOC(h->obs_q, sizeof(double) * obs_q.size());
    ALLOC(h->S.st4, sizeof(uint4) * n);
    ALLOC(h->S.ang, sizeof(double2) * n);
    ALLOC(h->S.ep, sizeof(int2) * n);
    ALLOC(h->S.mt, sizeof(uint32_t) * MT_STORE * (size_t)n);
    ALLOC(h->S.mc, sizeof(uint8_t) * MT_CODES * (size_t)n);
    ALLOC(h->eps, sizeof(tg_episode) * (size_t)h->eps_cap);
    ALLOC(h->eps_count, sizeof(int32_t));
    ALLOC(h->err, sizeof(uint32_t));
    return alloc_ctx(h->main, 0, n);
  };
  if (const int rc = alloc()) return cleanup(rc);
  L.gotab = h->gotab;
  L.masks = h->masks;
  L.obs_q = h->obs_q;
  h->L = L;
  if (hipMemcpy(h->grid, grid.data(), grid.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->genrand, gen, sizeof gen, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->gotab, gotab.data(), sizeof(uint32_t) * gotab.size(), hipMemcpyHostToDevice) != hipSuccess ||
      (h->masks && hipMemcpy(h->masks, masks.data(), sizeof(uint32_t) * masks.size(),
                             hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(h->obs_q, obs_q.data(), sizeof(double) * obs_q.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(h->eps_count, 0, sizeof(int32_t)) != hipSuccess ||
      hipMemset(h->err, 0, sizeof(uint32_t)) != hipSuccess)
    return cleanup(fail(TG_E_HIP, "tg_create: upload failed"));
  // seed -> generation 1 (first half) -> generation 2 (second half) -> the constructor's draws
  hipLaunchKernelGGL(k_create, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n,
                     seed_base + (uint64_t)global_offset, h->genrand);
  hipLaunchKernelGGL(k_gen_twist, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n,
                     MT_SEED_OFF, 0, 2 * MT_HALF_GENS);
  hipLaunchKernelGGL(k_reset, dim3(grid_for(n)), dim3(BLOCK), 0, 0, h->S, n, h->L,
                     (const uint8_t*)nullptr, (double*)nullptr, 0u);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return cleanup(fail(TG_E_HIP, "k_create: %s", hipGetErrorString(e)));
  *out = h;
  return TG_OK;
}
#undef ALLOC

void tg_destroy(tg_batch* h) {
  if (!h) return;
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != h->device) (void)hipSetDevice(h->device);
  if (h->srv_live) (void)srv_stop(h);
  srv_register(h, false);
  if (h->srv_trace && h->srv_calls)
    fprintf(stderr, "[serve] calls %lld launches %lld: mean per call %.2f us to post, %.2f us post -> "
            "answer, of which %.2f us between the server's pickup and its answer\n",
            (long long)h->srv_calls, (long long)h->srv_launches, h->srv_post_ns / h->srv_calls / 1e3,
            h->srv_rt_ns / h->srv_calls / 1e3, h->srv_gpu_ns / h->srv_calls / 1e3);
  if (h->srv_trace && h->srv_calls > 2) {  // server time = a + b * ticks (least squares)
    const double n = (double)h->srv_calls, sk = h->srv_fit[0], skk = h->srv_fit[1];
    const double sg = h->srv_gpu_ns, sgk = h->srv_fit[2];
    const double b = (n * sgk - sk * sg) / (n * skk - sk * sk), a = (sg - b * sk) / n;
    fprintf(stderr, "[serve] ticks per command %.2f; server time = %.2f us + %.3f us x ticks "
            "(GoTable in LDS: %d, %zu B)\n", sk / n, a / 1e3, b / 1e3, h->srv_stage, h->srv_dyn);
    if (h->srv_phase_n)
      fprintf(stderr, "[serve] py steps %lld, mean us: pickup -> option %.3f, option %.3f, observe "
              "%.3f, -> barrier %.3f, -> py_call return %.3f, -> answer %.3f\n",
              (long long)h->srv_phase_n, h->srv_phase[0] / h->srv_phase_n / 1e3,
              h->srv_phase[1] / h->srv_phase_n / 1e3, h->srv_phase[2] / h->srv_phase_n / 1e3,
              h->srv_phase[3] / h->srv_phase_n / 1e3, h->srv_phase[4] / h->srv_phase_n / 1e3,
              h->srv_phase[5] / h->srv_phase_n / 1e3);
  }
  if (h->srv_ev) (void)hipEventDestroy(h->srv_ev);
  if (h->srv_dep) (void)hipEventDestroy(h->srv_dep);
  if (h->srv_st) (void)hipStreamDestroy(h->srv_st);
  if (h->box) (void)hipHostFree(h->box);
  render_free(h->rs);
  flow_free(h);
  void* bufs[] = {h->grid, h->genrand, h->gotab, h->masks, h->obs_q, h->S.st4, h->S.ang, h->S.ep,
                  h->S.mt, h->S.mc, h->eps, h->eps_count, h->err, h->obs_scratch, h->kst,
                  h->mlp_params, h->mlp_actions};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  free_ctx(h->main);
  for (auto& c : h->grp) free_ctx(c);
  if (h->fork) (void)hipEventDestroy(h->fork);
  if (h->one) (void)hipHostFree(h->one);
  if (h->py) (void)hipHostFree(h->py);
  if (h->mask1) (void)hipHostFree(h->mask1);
  if (h->pyc) (void)hipFree(h->pyc);
  delete h;
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
  int rc = regen_all(h, 0);  // the old groups' pending lists
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (!h->grp.empty()) {  // the old groups' launch counters go on with the handle's own
    std::vector<unsigned long long> slot0(ST_COUNT);
    HIP_TRY(hipMemcpy(slot0.data(), h->main.stats, sizeof(unsigned long long) * ST_COUNT,
                      hipMemcpyDeviceToHost));
    for (auto& c : h->grp) {
      std::vector<unsigned long long> part((size_t)stat_slots(c.n) * ST_COUNT);
      HIP_TRY(hipMemcpy(part.data(), c.stats, sizeof(unsigned long long) * part.size(),
                        hipMemcpyDeviceToHost));
      for (size_t i = 0; i < part.size(); ++i) slot0[i % ST_COUNT] += part[i];
    }
    HIP_TRY(hipMemcpy(h->main.stats, slot0.data(), sizeof(unsigned long long) * ST_COUNT,
                      hipMemcpyHostToDevice));
  }
  for (auto& c : h->grp) free_ctx(c);
  h->grp.clear();
  h->stagger = stagger != 0;
  if (groups == 1) return TG_OK;
  if (!h->fork) HIP_TRY(hipEventCreateWithFlags(&h->fork, hipEventDisableTiming));
  // contiguous groups of whole 256-env workgroups
  const int64_t per = ((h->n + groups - 1) / groups + BLOCK - 1) / BLOCK * BLOCK;
  h->grp.resize((size_t)groups);
  for (int g = 0; g < groups; ++g) {
    const int64_t off = per * g, cnt = std::min(per, h->n - off);
    StepCtx& c = h->grp[(size_t)g];
    if (cnt <= 0 || (rc = alloc_ctx(c, off, cnt))) {
      for (auto& x : h->grp) free_ctx(x);
      h->grp.clear();
      return rc ? rc : fail(TG_E_INVAL, "tg_set_groups: empty group");
    }
    HIP_TRY(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
  }
  return TG_OK;
}

int tg_set_episode_capacity(tg_batch* h, int32_t cap) {
  BIND(h);
  if (cap < 1 || cap > (1 << 28)) return fail(TG_E_INVAL, "tg_set_episode_capacity: cap %d", cap);
  HIP_TRY(hipDeviceSynchronize());
  tg_episode* eps = nullptr;
  if (hipMalloc((void**)&eps, sizeof(tg_episode) * (size_t)cap) != hipSuccess)
    return fail(TG_E_NOMEM, "tg_set_episode_capacity: %d records", cap);
  (void)hipFree(h->eps);
  h->eps = eps;
  h->eps_cap = cap;
  HIP_TRY(hipMemset(h->eps_count, 0, sizeof(int32_t)));
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
  if (steps == 0) return TG_OK;
  if (const int rc = rollout_prep(h, "tg_rollout", steps,
                                  policy == TG_POLICY_UNIFORM || policy == TG_POLICY_MASKED, obs,
                                  reward, valid, done))
    return rc;
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
                      obs ? obs + (size_t)s * n * 9 : h->obs_scratch, obs ? n * 9 : 0,
                      reward + (size_t)s * n, valid + (size_t)s * n, done + (size_t)s * n,
                      action_seed, t0 + s, tb + (uint32_t)s};
      rc = launch_flow(h, k, io, ar, policy == TG_POLICY_MASKED ? 1 : 0, cs);
    }
    return rc;
  }
  return run_steps(h, steps, cs, [&](StepCtx& c, int32_t s, hipStream_t st, hipEvent_t mid) {
    const StepIO io{actions ? actions + (size_t)s * n : nullptr,
                    obs ? obs + (size_t)s * n * 9 : h->obs_scratch,
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
  if (const int rc = one_row(h)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (h->serve) {
    SrvBox c{};
    c.word = srv_word(SRV_STEP, action, false, false, 0);
    c.tstep = h->tstep++;
    if (const int rc = srv_call(h, c, st)) return rc;
  } else {
    TgOne* const d = h->one_dev;
    const StepIO io{nullptr, d->obs, &d->reward, &d->valid, &d->done, nullptr, POL_IMMEDIATE,
                    (uint64_t)(int64_t)action, 0, h->tstep++};
    const EpQueue q{h->eps, h->eps_count, h->eps_cap};
    hipLaunchKernelGGL((k_step<false, false, POL_IMMEDIATE>), dim3(1), dim3(BLOCK), 0, st, h->S,
                       h->n, h->L, h->grid, io, q, h->g0, h->main.stats, h->err, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  return row_out(h, obs, reward, valid, done);
}

int tg_available_mask1(tg_batch* h, uint16_t* mask, void* stream) {
  BIND_SERVE(h);
  if (h->n != 1 || !mask) return fail(TG_E_INVAL, "tg_available_mask1: a 1-env handle and a host output");
  if (h->serve) {
    SrvBox c{};
    c.word = srv_word(SRV_MASK, 0, false, false, 0);
    if (const int rc = srv_call(h, c, (hipStream_t)stream)) return rc;
    *mask = (uint16_t)h->box->mask;
    return TG_OK;
  }
  if (const int rc = pinned(h->mask1, h->mask1_dev, "tg_available_mask1", "result")) return rc;
  hipLaunchKernelGGL(k_mask, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->S, h->n, h->L, h->grid,
                     h->mask1_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *mask = *h->mask1;
  return TG_OK;
}

int tg_reset1(tg_batch* h, double* obs, void* stream) {
  BIND_SERVE(h);
  if (h->n != 1) return fail(TG_E_INVAL, "tg_reset1: a 1-env handle");
  if (h->serve) {
    SrvBox c{};
    c.word = srv_word(SRV_RESET, 0, false, false, 0);
    c.tstep = h->tstep;  // the next step's index: the new episode's start (as tg_reset)
    if (const int rc = srv_call(h, c, (hipStream_t)stream)) return rc;
  } else {
    if (const int rc = one_row(h)) return rc;
    hipLaunchKernelGGL(k_reset, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->S, h->n, h->L,
                       (const uint8_t*)nullptr, h->one_dev->obs, h->tstep);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  if (obs) memcpy(obs, h->one->obs, sizeof h->one->obs);
  return TG_OK;
}

int tg_set_serve(tg_batch* h, int on) {
  BIND(h);  // (stops a running server)
  h->serve = on != 0;
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
  if (obs) memcpy(obs, h->one->obs, sizeof h->one->obs);
  return TG_OK;
}

// ---- policies --------------------------------------------------------------------------------
int tg_policy_actions(tg_batch* h, uint64_t a0, int64_t t, int policy, int32_t* actions,
                      void* stream) {
  BIND(h);
  if (!actions || (policy != TG_POLICY_UNIFORM && policy != TG_POLICY_MASKED))
    return fail(TG_E_INVAL, "tg_policy_actions: bad arguments");
  hipLaunchKernelGGL(k_actions, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, h->grid, a0, h->g0, t, policy, actions);
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
  if (!h->mlp_params &&
      hipMalloc((void**)&h->mlp_params, sizeof(float) * (size_t)mlp_param_count(MLP_MAX_HIDDEN)) !=
          hipSuccess)
    return fail(TG_E_NOMEM, "tg_policy_mlp_load: parameter buffer");
  HIP_TRY(hipMemcpyAsync(h->mlp_params, params_dev, sizeof(float) * (size_t)mlp_param_count(hidden),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  h->mlp_hidden = hidden;
  h->mlp_act = act;
  h->mlp_masked = masked ? 1 : 0;
  return TG_OK;
}

int tg_policy_mlp(tg_batch* h, uint64_t a0, int64_t t, int32_t mode, int32_t* actions, float* logp,
                  float* value, float* logits, void* stream) {
  BIND(h);
  if (!h->mlp_hidden) return fail(TG_E_STATE, "tg_policy_mlp: no parameters (tg_policy_mlp_load)");
  if (!actions || (mode != TG_MLP_SAMPLE && mode != TG_MLP_GREEDY))
    return fail(TG_E_INVAL, "tg_policy_mlp: bad arguments");
  return launch_policy_mlp(h, 0, h->n, a0, t, mode, actions, logp, value, logits,
                           (hipStream_t)stream);
}

int tg_rollout_mlp(tg_batch* h, int32_t steps, uint64_t a0, int64_t t0, int32_t mode, uint32_t flags,
                   int32_t* actions, double* obs, int32_t* reward, uint8_t* valid, uint8_t* done,
                   float* logp, float* value, void* stream) {
  BIND(h);
  if (!h->mlp_hidden) return fail(TG_E_STATE, "tg_rollout_mlp: no parameters (tg_policy_mlp_load)");
  if (h->mode == TG_MODE_FLOW)
    return fail(TG_E_INVAL, "tg_rollout_mlp: TG_MODE_FLOW evaluates its policy inside k_flow; use "
                            "TG_MODE_COMPACT or TG_MODE_DIRECT");
  if (steps == 0) return TG_OK;
  if (const int rc = rollout_prep(h, "tg_rollout_mlp", steps,
                                  mode == TG_MLP_SAMPLE || mode == TG_MLP_GREEDY, obs, reward, valid,
                                  done))
    return rc;
  const int64_t n = h->n;
  if (!actions && !h->mlp_actions)  // the step kernels always read an action row
    if (hipMalloc((void**)&h->mlp_actions, sizeof(int32_t) * (size_t)n) != hipSuccess)
      return fail(TG_E_NOMEM, "tg_rollout_mlp: action scratch");
  const bool ar = (flags & TG_STEP_AUTORESET) != 0;
  const uint32_t tb = h->tstep;
  h->tstep += (uint32_t)steps;
  // step s of a stepper: the actor into row s, then the step kernels with those actions given
  return run_steps(h, steps, (hipStream_t)stream,
                   [&](StepCtx& c, int32_t s, hipStream_t st, hipEvent_t mid) {
    int32_t* const act = actions ? actions + (size_t)s * n : h->mlp_actions;
    const int rc = launch_policy_mlp(h, c.off, c.n, a0, t0 + s, mode, act,
                                     logp ? logp + (size_t)s * n : nullptr,
                                     value ? value + (size_t)s * n : nullptr, nullptr, st);
    if (rc) return rc;
    const StepIO io{act, obs ? obs + (size_t)s * n * 9 : h->obs_scratch, reward + (size_t)s * n,
                    valid + (size_t)s * n, done + (size_t)s * n, nullptr, -1, 0, 0};
    return launch_step(h, c, io, ar, st, tb + (uint32_t)s, mid);
  });
}

// ---- state in and out ------------------------------------------------------------------------
int tg_available_mask(tg_batch* h, uint16_t* mask, void* stream) {
  BIND(h);
  if (!mask) return fail(TG_E_INVAL, "tg_available_mask: null output");
  hipLaunchKernelGGL(k_mask, dim3(grid_for(h->n)), dim3(BLOCK), 0, (hipStream_t)stream, h->S,
                     h->n, h->L, h->grid, mask);
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
  hipLaunchKernelGGL(k_drain_episodes, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->eps,
                     h->eps_count, h->eps_cap, out, count, cap);
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
      const uint4 s = st[(size_t)i];
      if (pos) {
        pos[2 * i] = (int16_t)(s.x & 0xFFFFu);
        pos[2 * i + 1] = (int16_t)(s.x >> 16);
      }
      if (flags) flags[i] = s.y;
      if (objs) {
        objs[4 * i] = (int8_t)(s.z & 0xFF);
        objs[4 * i + 1] = (int8_t)((s.z >> 8) & 0xFF);
        objs[4 * i + 2] = (int8_t)((s.z >> 16) & 0xFF);
        objs[4 * i + 3] = (int8_t)(s.z >> 24);
      }
    }
  }
  if (ang) HIP_TRY(hipMemcpy(ang, h->S.ang, sizeof(double2) * n, hipMemcpyDeviceToHost));
  if (ep) {  // (return, start step) -> (return, length): the steps since the start
    HIP_TRY(hipMemcpy(ep, h->S.ep, sizeof(int2) * n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) ep[2 * i + 1] = (int32_t)(h->tstep - (uint32_t)ep[2 * i + 1]);
  }
  if (mt_pos) {
    // CPython's index into the generation holding the position
    for (int64_t i = 0; i < n; ++i) mt_pos[i] = (st[(size_t)i].w & MT_POS_MASK) % MT_N;
  }
  if (mt) {
    // the generations, gathered on the device into a bounded staging buffer (<= 64 Ki envs,
    // 160 MB) and copied out in one transfer per chunk
    const int64_t chunk = n < (1 << 16) ? n : (1 << 16);
    uint32_t* stage = nullptr;
    if (hipMalloc((void**)&stage, sizeof(uint32_t) * MT_N * (size_t)chunk) != hipSuccess)
      return fail(TG_E_NOMEM, "tg_read_state: staging buffer");
    int rc = TG_OK;
    for (int64_t first = 0; first < n && rc == TG_OK; first += chunk) {
      const int64_t cnt = n - first < chunk ? n - first : chunk;
      const int64_t threads = cnt * (MT_N / 4);
      hipLaunchKernelGGL(k_gather_mt, dim3((unsigned)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK),
                         0, 0, h->S, first, cnt, stage);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpy(mt + first * MT_N, stage, sizeof(uint32_t) * MT_N * (size_t)cnt,
                      hipMemcpyDeviceToHost);
      if (e != hipSuccess) rc = fail(TG_E_HIP, "tg_read_state: %s", hipGetErrorString(e));
    }
    (void)hipFree(stage);
    if (rc) return rc;
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
    uint4 w;
    w.x = ((uint32_t)e.px & 0xFFFFu) | ((uint32_t)e.py << 16);
    w.y = e.f;
    w.z = ((uint32_t)e.kx & 0xFF) | (((uint32_t)e.ky & 0xFF) << 8) | (((uint32_t)e.gx & 0xFF) << 16) |
          ((uint32_t)e.gy << 24);
    w.w = e.mti;
    st[(size_t)i] = w;
  }
  HIP_TRY(hipDeviceSynchronize());
  // validated: the pending refill lists name the old states' halves, and every ring is rebuilt
  h->main.rpend = 0;
  for (auto& c : h->grp) c.rpend = 0;
  HIP_TRY(hipMemset(h->main.regen_ctr, 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
  for (auto& c : h->grp) HIP_TRY(hipMemset(c.regen_ctr, 0, sizeof(int32_t) * 2 * RCTR_N * CTR_STRIDE));
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

// ---- diagnostics and measurement -------------------------------------------------------------
int tg_errors(tg_batch* h, uint32_t* out, void* stream) {
  BIND(h);
  if (!out) return fail(TG_E_INVAL, "tg_errors: null output");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_errors, dim3(grid_for(h->n)), dim3(BLOCK), 0, st, h->S.st4, h->n, h->err);
  HIP_TRY(hipGetLastError());
  uint32_t v = 0;
  HIP_TRY(hipMemcpyAsync(&v, h->err, sizeof v, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out = v;
  return TG_OK;
}

int tg_set_timing(tg_batch* h, int every) {
  BIND(h);
  if (every < 0) return fail(TG_E_INVAL, "tg_set_timing: every %d < 0", every);
  HIP_TRY(hipDeviceSynchronize());
  int rc = flush_timing(h);  // records of the previous setting are kept in the sums
  if (rc) return rc;
  if (every && !h->kst && (rc = kst_reset(h))) return rc;
  h->timing_every = every;
  h->timing_calls = 0;
  return TG_OK;
}

int tg_get_stats(tg_batch* h, tg_stats* out) {
  BIND(h);
  if (!out) return fail(TG_E_INVAL, "tg_get_stats: null output");
  HIP_TRY(hipDeviceSynchronize());
  int rc = flush_timing(h);
  if (rc) return rc;
  unsigned long long s[ST_COUNT] = {};
  std::vector<StepCtx*> ctxs{&h->main};
  for (auto& c : h->grp) ctxs.push_back(&c);
  for (StepCtx* c : ctxs) {
    const size_t nb = (size_t)stat_slots(c->n);
    std::vector<unsigned long long> part(nb * ST_COUNT);
    HIP_TRY(hipMemcpy(part.data(), c->stats, sizeof(unsigned long long) * part.size(),
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
  out->kernel_ms = h->kernel_ms_done;
  out->regens = (int64_t)s[ST_REGENS] * MT_HALF_GENS;  // halves -> generations
  out->regens_quiet = (int64_t)s[ST_RQUIET] * MT_HALF_GENS;
  out->wave_ticks = (int64_t)s[ST_WTICKS];
  out->timed_launches = h->timed_launches;
  out->run_ms = h->run_ms_done;
  out->regen_ms = h->regen_ms_done;
  out->regen_timed = h->regen_timed;
  out->regen_launches = h->regen_launches;
  out->classify_ms = h->classify_ms_done;
  return TG_OK;
}

int tg_stats_reset(tg_batch* h) {
  BIND(h);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(h->main.stats, 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(h->n)));
  for (auto& c : h->grp)
    HIP_TRY(hipMemset(c.stats, 0, sizeof(unsigned long long) * ST_COUNT * (size_t)stat_slots(c.n)));
  if (h->kst) {
    const int rc = kst_reset(h);  // drops the unflushed records
    if (rc) return rc;
  }
  h->kernel_ms_done = 0.0;
  h->run_ms_done = 0.0;
  h->classify_ms_done = 0.0;
  h->timed_launches = 0;
  h->regen_ms_done = 0.0;
  h->regen_timed = 0;
  h->regen_launches = 0;
  return TG_OK;
}

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
                     (hipStream_t)stream, h->L, h->grid, x0, x1, y0, y1, door_bits, out);
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
