// tg_batch.h — the handle behind include/tg_amd.h, shared by the step (tg_amd.hip; tg_flow.hip
// through tg_dev.h, for Soa) and render (tg_render.hip) translation units of libtg_amd.so.
// Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tg_amd.h"
#include "tg_state.h"
#include "tg_srv_word.h"

namespace tg {

extern thread_local std::string g_err;  // tg_last_error() text (tg_amd.hip)
inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail(TG_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
// leave the calling function with a failed step's error code (fail() has the text)
#define TG_TRY(expr)                        \
  do {                                      \
    if (const int rc_ = (expr)) return rc_; \
  } while (0)

struct Soa {
  uint4* st4;
  double2* ang;
  int2* ep;
  uint32_t* mt;   // [N][MT_STORE]: the ring's even generations (tg_mt.h)
  uint8_t* mc;    // [N][MT_CODES]: the draw codes of the ring's generations (tg_mt.h draw_code)
};

// tg_step1's result row (one env)
struct TgOne {
  double obs[9];
  int32_t reward;
  uint8_t valid, done;
};
static_assert(sizeof(TgOne) == 80, "TgOne: ten 8-B words (k_serve1 copies it out by word)");

// The N = 1 server's mailbox (k_serve1, tg_py1.h): pinned, coherent host memory (line 2:
// TG_SERVE_TRACE's stamps).  Line 0 is
// the host's: a command is one 16-B group (seq last: the server reads the group with one load,
// and a group whose seq is new carries the command's fields) and, for a reset, gauss_next
// (read after the group).  Line 1 is the server's: done, the last command it served (a server
// that starts reads it, so a command posted while none ran is served by the next one).
struct SrvBox {
  uint32_t word;        // srv_word (tg_srv_word.h: the kinds, the encoder and the decoders)
  uint32_t tstep;       // the step's index (h->tstep)
  uint32_t pad0;
  uint32_t seq;         // the last command posted (written last)
  uint64_t gauss_bits;  // SRV_RESET_PY: the caller's gauss_next
  uint8_t pad1[64 - 24];
  uint32_t done;
  uint32_t mask;           // SRV_MASK's answer: available_mask's bits
  uint32_t pad2[2];
  uint64_t t_seen, t_end;  // TG_SERVE_TRACE: the server's clock at the command's pickup / answer
  uint32_t ticks;          //   and the command's ticks
  uint32_t pad3[7];
  uint64_t phase[5];       // TG_SERVE_TRACE: py_call's phase stamps (SRV_STEP_PY)
  uint64_t pad4[3];
};
static_assert(sizeof(SrvBox) == 192, "SrvBox: three 64-B lines");

// ---- owners -------------------------------------------------------------------------------------
// Every device buffer, pinned buffer, stream and event of the library is held by one of the four
// move-only types below and released by its destructor; nothing else calls a HIP free / destroy.
// They are host objects: a kernel takes get() (or dev()), never an owner (a copy does not
// compile).  g_live counts the resources held in this process (tg_live_resources).
extern std::atomic<int64_t> g_live;  // tg_amd.hip

template <class H, hipError_t (*Release)(H)>
class Owner {
 public:
  Owner() = default;
  Owner(Owner&& o) noexcept : h_(o.h_) { o.h_ = H{}; }
  Owner& operator=(Owner&& o) noexcept {  // (what it held goes with `o`)
    std::swap(h_, o.h_);
    return *this;
  }
  ~Owner() { reset(); }
  void reset() {
    if (!h_) return;
    (void)Release(h_);
    h_ = H{};
    g_live.fetch_sub(1, std::memory_order_relaxed);
  }
  explicit operator bool() const { return h_ != H{}; }

 protected:
  void adopt(H h) {  // (after reset)
    h_ = h;
    g_live.fetch_add(1, std::memory_order_relaxed);
  }
  H h_{};
};

template <class T>
class DevBuf : public Owner<void*, hipFree> {
 public:
  // `count` Ts of device memory in place of what it held (contents undefined)
  int alloc(size_t count, const char* what) {
    reset();
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * count) != hipSuccess) {
      (void)hipGetLastError();  // reported here: not left for a later launch's check to find
      return fail(TG_E_NOMEM, "hipMalloc %zu B for %s", sizeof(T) * count, what);
    }
    adopt(p);
    return TG_OK;
  }
  // alloc, then a synchronous copy of `count` Ts from host memory
  int upload(const void* src, size_t count, const char* what) {
    TG_TRY(alloc(count, what));
    HIP_TRY(hipMemcpy(h_, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return TG_OK;
  }
  T* get() const { return static_cast<T*>(h_); }
};

// one T of pinned, coherent host memory the device writes, and its device-side address
template <class T>
class PinnedBuf : public Owner<void*, hipHostFree> {
 public:
  int alloc(const char* what) {  // zeroed; a no-op while it holds one (allocated at first use)
    if (h_) return TG_OK;
    void* p = nullptr;
    if (hipHostMalloc(&p, sizeof(T), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TG_E_NOMEM, "pinned %s", what);
    }
    adopt(p);
    memset(p, 0, sizeof(T));
    if (hipHostGetDevicePointer(&dev_, p, 0) != hipSuccess) {
      reset();
      return fail(TG_E_HIP, "pinned %s: no device address", what);
    }
    return TG_OK;
  }
  T* get() const { return static_cast<T*>(h_); }
  T* operator->() const { return get(); }
  T* dev() const { return h_ ? static_cast<T*>(dev_) : nullptr; }

 private:
  void* dev_ = nullptr;
};

struct Stream : Owner<hipStream_t, hipStreamDestroy> {
  int create() {  // non-blocking; a no-op while it holds one
    if (h_) return TG_OK;
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    adopt(s);
    return TG_OK;
  }
  hipStream_t get() const { return h_; }
};
struct Event : Owner<hipEvent_t, hipEventDestroy> {
  int create() {  // untimed; a no-op while it holds one
    if (h_) return TG_OK;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    adopt(e);
    return TG_OK;
  }
  hipEvent_t get() const { return h_; }
};

struct RenderState;  // tg_render.hip
void render_free(RenderState* rs);
struct RenderDelete {
  void operator()(RenderState* rs) const { render_free(rs); }
};

// One stepper over envs [off, off + n) of the handle: its worklists, counters, refill lists and
// launch counters.  The handle's own covers every env (tg_step, tg_rollout); with tg_set_groups
// each group has one, and tg_rollout steps the groups on streams of their own (tg_amd.hip).
struct StepCtx {
  int64_t off = 0, n = 0;
  DevBuf<unsigned long long> stats;  // [stat_slots(n)][ST_COUNT] launch counters
  DevBuf<int32_t> wl;    // per-(option, shard) worklists (compact mode)
  DevBuf<uint4> wst4;    // the listed envs' state in worklist order (k_classify -> k_run)
  DevBuf<double2> wang;
  DevBuf<int2> wep;
  DevBuf<int32_t> wctr;  // sharded counters (worklists, quiet lists), two sets (step parity)
  DevBuf<uint32_t> refill;  // stale MT halves listed by k_classify: SHARDS lists (k_regen)
  int64_t rcap = 0;         // entries per list: a shard's envs x REGEN_STEPS
  int64_t shard_cap = 0;
  DevBuf<uint32_t> quiet;   // this step's quiet envs' stale halves: SHARDS lists (k_run's drain)
  int64_t qcap = 0;         // entries per list: a shard's envs
  int parity = 0;  // which half of wctr this compact step counts in
  int rpend = 0;   // compact steps whose refill lists k_regen has not drained
  DevBuf<int32_t> regen_ctr;  // per XCD: k_regen's grab counters and the lists' lengths, two
                              // sets (k_regen zeroes the other set for the next launch)
  int regen_parity = 0;       // which set the next k_regen counts in
  // tg_rollout_mlp_gae: the saved states of the envs k_timelimit is about to reset (k_trunc_list;
  // allocated at first use): 4 n entries, which bounds what 4 x limit steps can append
  DevBuf<uint4> tst4;
  DevBuf<double2> tang;
  DevBuf<int64_t> tdst;
  DevBuf<int32_t> tcnt;       // the list's length, two words: one per use of the list, in turn
  int tparity = 0;            // which word of tcnt the list counts in now
  int64_t twin = 0;           // steps appended since k_value_mlp last ran over the list
  Stream st;                  // a group's stream (groups only)
  Event ev;                   //   and its join event
};

// tg_set_timing's state: the in-kernel span records of the timed launches and their sums
struct Timing {
  int every = 0;        // timing of every k-th step launch (0: off)
  uint64_t calls = 0;   // step launches since timing was enabled
  DevBuf<unsigned long long> kst;  // the records (tg_amd.hip)
  int kst_steps = 0, kst_regens = 0;  // records in use
  std::vector<int> kst_k;          // steps each in-use step record covers (a k_flow launch: K)
  struct Sums {  // of the flushed records (tg_get_stats; zeroed by tg_stats_reset)
    double kernel_ms = 0.0;    // the timed step launches' kernel spans
    double classify_ms = 0.0;  //   of which k_classify
    double run_ms = 0.0;       //   and k_run (or k_step)
    int64_t timed_launches = 0;
    double regen_ms = 0.0;       // the timed k_regen launches' spans
    int64_t regen_launches = 0;  // k_regen launches (timed or not)
    int64_t regen_timed = 0;
  } sums;
};

// the learned actor (tg_policy_mlp_load): its packed parameters (sized for the widest network at
// the first load and never reallocated), hidden width (0: none loaded), TG_ACT_*, masking
struct Mlp {
  DevBuf<float> params;
  int hidden = 0, act = 0, masked = 0;
  DevBuf<int32_t> actions;  // tg_rollout_mlp without an actions output
  DevBuf<float> vboot;      // tg_rollout_mlp_gae without a vboot output
};

// TG_MODE_FLOW's work structures (tg_flow.h Flow; allocated at the first flow rollout)
struct FlowState {
  bool ready = false;
  int P = 0;                // sub-problems: the XCDs the census saw
  uint32_t xmap = 0;        // XCC id -> sub-problem (nibbles)
  int32_t C = 0;            // 64-env chunks
  int64_t qcap = 0, jcap = 0, lcap = 0;
  DevBuf<int32_t> ctl[2];   // two parities: a launch zeroes the other's
  DevBuf<uint32_t> q[2];
  DevBuf<int32_t> fill[2];
  DevBuf<int32_t> list, outst;
  int parity = 0;
  int bpc[2][2] = {{0, 0}, {0, 0}};  // k_flow<AR, POL> workgroups per CU (occupancy API)
  int64_t launches = 0;
};

// What exists only for a 1-env handle: the N = 1 calls' buffers (allocated at first use) and
// their resident server (k_serve1): tg_step1 / tg_step1_py / tg_reset1_py post a command to its
// mailbox and spin on the answer instead of a launch and a synchronisation each; every other
// entry point stops it first (BIND).
struct One {
  PinnedBuf<TgOne> row;        // tg_step1's result row, which the kernel writes
  PinnedBuf<uint16_t> mask1;   // tg_available_mask1's answer without the server
  PinnedBuf<tg_pystate> py;    // tg_step1_py / tg_reset1_py's stream state
  DevBuf<uint32_t> pyc;        // the Python stream's generation + 2 successors, on the device
  tg_pystate py_last{};        // the state the last tg_*1_py call returned
  bool py_warm = false;        // pyc matches py_last
  bool serve = true;           // tg_set_serve / TG_SERVE (read at tg_create)
  uint32_t idle = 0;           // the server leaves after this many 10-ns ticks without a command
  PinnedBuf<SrvBox> box;       // the mailbox
  Stream st;                   // the server's stream: after the caller's stream (dep)
  Event ev;                    //   recorded after each server launch: complete = it left
  Event dep;
  bool live = false;           // a server was launched and not stopped
  uint32_t seq = 0;
  int64_t t_last = 0;          // host clock (ns) at the last answer
  int64_t launches = 0, calls = 0;
  int stage = -1;              // the level tables the server keeps in LDS (k_serve1 stage; -1:
  size_t dyn = 0;              //   not chosen yet) and their dynamic LDS bytes
  struct Trace {               // TG_SERVE_TRACE: sums printed at tg_destroy (diagnostic)
    bool on = false;
    double rt_ns = 0.0, gpu_ns = 0.0, post_ns = 0.0, fit[3] = {0.0, 0.0, 0.0};
    double phase[6] = {0, 0, 0, 0, 0, 0};
    int64_t phase_n = 0;
  } trace;

  int need_row() { return row.alloc("N = 1 result row"); }
  int need_py();      // py and pyc (tg_amd.hip)
  int need_server();  // every buffer, the stream and the events a server uses (tg_amd.hip)
  // every buffer of this struct the server may write is allocated, whichever call launches it
  bool server_ready() const { return box.dev() && py.dev() && pyc.get() && row.dev() && st && ev && dep; }
};

}  // namespace tg

// a snapshot (tg_amd.h tg_snap): `slots` saved envs of the handle that created it, one array per
// field of a slot (tg_snapshot.h Snap).  The handle owns it (tg_batch::snaps).
struct tg_snap {
  tg_batch* owner = nullptr;
  int64_t slots = 0;
  tg::DevBuf<uint4> st4;
  tg::DevBuf<double2> ang;
  tg::DevBuf<int2> ep;
  tg::DevBuf<uint32_t> mt;  // [slots][624]
};

// the handle (tg_amd.h tg_batch).  Members are destroyed in reverse order after tg_destroy has
// stopped the server: nothing on the device runs against a buffer that is being freed.
struct tg_batch {
  int device = 0;
  int cus = 0;  // compute units
  int64_t n = 0;
  int64_t g0 = 0;
  uint64_t seed0 = 0;
  // the level: the kernels' view L and the tables it points into
  tg::Level L{};
  tg::DevBuf<uint32_t> grid;  // bordered cell grid, padded to whole words
  tg::DevBuf<uint32_t> genrand;
  tg::DevBuf<uint32_t> gotab;  // GoTable (tg_rules.h go_lookup): W * H * 32 entries
  tg::DevBuf<uint32_t> masks;  // the level bitmasks (tg_map.h Map::mk), or none
  tg::DevBuf<double> obs_q;    // get_state's quotient table (tg_state.h Level::obs_q)
  std::string domain;          // domain.txt text (the renderer's cell sprites)
  // the envs: the kernels' view S and the arrays it points to
  tg::Soa S{};
  struct {
    tg::DevBuf<uint4> st4;
    tg::DevBuf<double2> ang;
    tg::DevBuf<int2> ep;
    tg::DevBuf<uint32_t> mt;
    tg::DevBuf<uint8_t> mc;
  } env;
  tg::DevBuf<tg_episode> eps;  // the completed-episode queue (tg_episodes)
  tg::DevBuf<int32_t> eps_count;
  int32_t eps_cap = 0;
  tg::DevBuf<uint32_t> err;
  tg::DevBuf<double> obs_scratch;  // tg_rollout without an obs output
  // the steppers
  int mode = TG_MODE_COMPACT;
  tg::StepCtx main;                // the stepper over every env
  std::vector<tg::StepCtx> grp;    // tg_set_groups: the groups' steppers (tg_rollout)
  tg::Event fork;                  //   the groups' fork event
  bool stagger = false;            //   group g + 1 starts after group g's first k_classify
  uint32_t tstep = 0;  // steps taken by the handle (mod 2^32): S.ep holds each episode's start step
  uint32_t time_limit = 0;  // tg_set_time_limit: k_timelimit after every step's kernels (0: off)
  int regen_per_cu = 0;  // k_regen workgroups resident per CU (occupancy API, first use)
  tg::Timing tm;
  tg::Mlp mlp;
  tg::One one;
  std::unique_ptr<tg::RenderState, tg::RenderDelete> rs;  // tg_render_init
  tg::FlowState fl;
  std::vector<std::unique_ptr<tg_snap>> snaps;  // tg_snap_create's, until tg_snap_destroy
  // read once at tg_create: TG_FLOW_DEBUG (print the census and every k_flow launch's
  // sub-problem counters; synchronises after each launch) and the test hook TG_FLOW_SKIP_PART
  // (sub-problem x's waves leave at once: tests/test_gpu_flow.py checks TG_ERR_FLOW is raised)
  bool flow_debug = false;
  int flow_skip = -1;
};

namespace tg {
inline int bind(const tg_batch* h) {
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != h->device) HIP_TRY(hipSetDevice(h->device));
  return TG_OK;
}
int srv_stop(tg_batch* h);  // tg_amd.hip: stop the N = 1 server (if one runs) and wait for it
// every entry point: the handle's device current, and the N = 1 server stopped (it steps the
// env on a stream of its own: nothing else may touch the handle's state while it runs)
#define BIND(h)                       \
  do {                                \
    if (!(h)) return fail(TG_E_INVAL, "null handle"); \
    int rc_ = bind(h);                \
    if (!rc_ && (h)->one.live) rc_ = srv_stop(h); \
    if (rc_) return rc_;              \
  } while (0)
// the N = 1 calls the server serves
#define BIND_SERVE(h)                 \
  do {                                \
    if (!(h)) return fail(TG_E_INVAL, "null handle"); \
    int rc_ = bind(h);                \
    if (rc_) return rc_;              \
  } while (0)

}  // namespace tg
