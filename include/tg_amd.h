/* tg_amd.h — C ABI of the MI355X batched Treasure Game simulator (libtg_amd.so).
 *
 * This is the drop-in boundary for the reference env's hot path.  One handle owns a batch of
 * N independent envs resident in HBM (struct-of-arrays state + one CPython-compatible
 * MT19937 stream per env).  Env g of a handle created with (seed_base, global_offset) is
 * bit-identical to the reference env made by
 *     random.seed(seed_base + global_offset + g); env = TreasureGame()
 * and replays the reference's reset()/step()/available_mask on the same calls.
 *
 * Conventions
 *   - every buffer argument is a DEVICE pointer on the handle's device (caller-owned);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is
 *     asynchronous on that stream unless documented otherwise, and calls on one handle must
 *     be serialised by the caller (one handle = one stream, not re-entrant);
 *   - functions return TG_OK (0) or a negative TG_E* code; tg_last_error() gives the text
 *     (thread-local);
 *   - no torch or HIP types appear here.
 *
 * Reference interfaces replaced (paths under gym_treasure_game/envs/ of the reference):
 *   tg_create          TreasureGame.__init__            treasure_game.py:63-76
 *   tg_reset           TreasureGame.reset               treasure_game.py:78-81
 *   tg_step            TreasureGame.step                treasure_game.py:91-96
 *                        -> _Option.run              _treasure_game_impl/_option.py:20-36
 *                        -> _TreasureGameImpl.step   _treasure_game_impl/_treasure_game_impl.py:290-359
 *   tg_available_mask  TreasureGame.available_mask      treasure_game.py:83-89
 *   tg_render          TreasureGame.render('rgb_array')  treasure_game.py:98-105
 *                        -> _TreasureGameDrawer.draw_domain _treasure_game_impl/
 *                           _treasure_game_drawer.py:136-163, draw_object :238-269
 *                      (ObservationWrapper, treasure_game.py:38-51, renders every reset/step)
 *   obs layout         _TreasureGameImpl.get_state      _treasure_game_impl.py:368-378
 *   level text         the 3 level files read by        _treasure_game_impl.py:75-202
 */
#ifndef TG_AMD_H
#define TG_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_OK 0
#define TG_E_INVAL (-1)    /* bad argument / level */
#define TG_E_HIP (-2)      /* HIP runtime error */
#define TG_E_NOMEM (-3)    /* device allocation failed */
#define TG_E_NODEV (-4)    /* no usable gfx950 device */
#define TG_E_STATE (-5)    /* an env hit an error flag (see tg_errors) */

#define TG_OBS_DIM 9       /* playerx, playery, handle1.angle, handle2.angle, key.x, key.y,
                              bolt.locked, goldcoin.x, goldcoin.y (IM/:380-400) */
#define TG_NUM_ACTIONS 9   /* go_left, go_right, up_ladder, down_ladder, interact, down_left,
                              down_right, jump_left, jump_right (IM/:495) */

/* per-env error bits reported by tg_errors() */
#define TG_ERR_TICKCAP (1u << 24)  /* an option ran > 16384 ticks (the reference would loop) */
#define TG_ERR_BAG (1u << 25)      /* bag overflow */
#define TG_ERR_ACTION (1u << 26)   /* action outside [-9, 8]: the reference raises IndexError */
#define TG_ERR_NEARINT (1u << 27)  /* reset gauss within 1e-9 of an int() boundary (libm watch) */
#define TG_ERR_RENDER (1u << 28)   /* render: a handle shaft end point within 1e-9 of an int()
                                      boundary (libm watch), or a shaft off the screen */
#define TG_ERR_WINDOW (1u << 29)  /* a lane drew past its staged draw codes (a bound broken: bug) */
#define TG_ERR_FLOW (1u << 30)    /* TG_MODE_FLOW: a k_flow wait ran past its 4-s bound (a bug; the
                                      launch ended early, its results are not valid) */

/* step flags */
#define TG_STEP_AUTORESET 1u       /* reset() an env right after a step that returned done */

/* bits of a done row (tg_step, tg_rollout, tg_rollout_mlp) */
#define TG_DONE_TERMINATED 1u      /* the env's own end (TG/:95); the only bit without a step limit */
#define TG_DONE_TRUNCATED 2u       /* the episode reached tg_set_time_limit's limit in this step */
/* in tg_episode.len: the episode was ended by the step limit, not by the env */
#define TG_EPISODE_TRUNCATED (1 << 30)

/* action policies of tg_policy_actions */
#define TG_POLICY_UNIFORM 0        /* a = h(action_seed, g, t) % 9 (action_space.sample stand-in) */
#define TG_POLICY_MASKED 1         /* k-th set bit of available_mask, k = h % popcount */

typedef struct tg_batch tg_batch;

/* Completed episode record written by an auto-reset step. */
typedef struct {
  int64_t env;      /* global env index (global_offset + local index) */
  int32_t ret;      /* sum of step rewards since the last reset (None counts 0) */
  int32_t len;      /* env-steps since the last reset, | TG_EPISODE_TRUNCATED if the step limit
                       ended it (tg_set_time_limit) */
} tg_episode;

/* A Python-level random stream's state, as random.getstate() holds it (CPython random.py
 * getstate: (3, tuple of 624 MT19937 words + index, gauss_next)): the reference's envs all draw
 * from the process-global `random` (_treasure_game_impl.py:2, _objects.py:9). */
typedef struct {
  uint32_t mt[624];   /* the generation CPython's genrand_uint32 reads */
  uint32_t index;     /* its next word, 0..624 (624: twist before the next word) */
  uint32_t has_gauss; /* gauss_next is not None */
  double gauss_next;
} tg_pystate;

/* Counters accumulated over all tg_step calls since creation / tg_stats_reset. */
typedef struct {
  int64_t steps;        /* env-steps (one per env per tg_step) */
  int64_t valid_steps;  /* steps whose option could run (reward not None) */
  int64_t ticks;        /* primitive ticks (_TreasureGameImpl.step calls) */
  int64_t draws;        /* random() draws (2 MT words each) */
  int64_t episodes;     /* completed episodes (auto-reset) */
  int64_t episodes_dropped; /* records lost because the queue (max(4N, 65536)) was full */
  int64_t launches;     /* step-kernel launches */
  double kernel_ms;     /* summed kernel time of the timed step launches (tg_set_timing): each
                           kernel's span from its first wave's start to its last wave's end, by
                           in-kernel s_memrealtime stamps (100 MHz); nothing goes on the stream */
  int64_t regens;       /* MT19937 generations regenerated by the step kernels (624 words +
                           312 random() values each) */
  int64_t wave_ticks;   /* sum over the tick loops' wavefronts of their longest lane's ticks:
                           lane efficiency = ticks / (64 * wave_ticks) (an upper bound for the
                           go loops, whose lanes may also wait for the others' plain ticks) */
  int64_t timed_launches; /* launches timed (tg_set_timing) */
  double run_ms;        /* of kernel_ms, the second kernel (k_run in the compact mode; the single
                           kernel of the direct launches) */
  double regen_ms;      /* summed span of the k_regen launches while timing is on */
  int64_t regen_timed;  /* k_regen launches timed (while tg_set_timing is on) */
  int64_t regen_launches; /* k_regen launches (deferred MT regenerations, tg_regenerate) */
  double classify_ms;   /* of kernel_ms, k_classify */
  int64_t regens_quiet; /* of regens, the generations regenerated inside k_run by its waves without
                           a chunk: the stale halves of envs whose option could not run in the step
                           that listed them (compact mode; the rest are k_regen's, or the lanes') */
  int64_t episodes_truncated; /* of episodes, those the step limit ended (tg_set_time_limit) */
} tg_stats;

/* Create N envs on `device`: env i is `random.seed(seed_base + global_offset + i);
 * TreasureGame()` (the constructor consumes 4 draws; call tg_reset for env.reset(), as with
 * the reference; seed_base + global_offset + N - 1 must not exceed 2^64 - 1).  Level text in
 * the reference's file formats (domain.txt,
 * domain-objects.txt, domain-interactions.txt); NULL for all three = the built-in default
 * level.  Synchronises. */
int tg_create(tg_batch **out, int64_t num_envs, uint64_t seed_base, int64_t global_offset,
              int device, const char *domain_txt, const char *objects_txt,
              const char *interactions_txt);
void tg_destroy(tg_batch *h);

int64_t tg_num_envs(const tg_batch *h);

/* reset(): all envs (mask == NULL) or those with mask[i] != 0; writes obs [N][9] f64 for
 * every env (current obs for the ones not reset).  obs may be NULL. */
int tg_reset(tg_batch *h, const uint8_t *mask, double *obs, void *stream);

/* step(a) for every env: actions int32 [N] in [-9, 8] (Python list indexing).  Outputs:
 * obs f64 [N][9], reward int32 [N] (0 when not valid), valid u8 [N] (0 == reward None),
 * done u8 [N].  flags: TG_STEP_AUTORESET; then final_obs (may be NULL) receives the pre-reset
 * obs of every env (== obs where no reset happened) and completed episodes are appended to
 * the handle's episode buffer (tg_episodes). */
int tg_step(tg_batch *h, const int32_t *actions, double *obs, int32_t *reward, uint8_t *valid,
            uint8_t *done, double *final_obs, uint32_t flags, void *stream);

/* step(action) of a 1-env handle, for the N=1 drop-in (TreasureGame.step, TG/:91-96), no
 * auto-reset (as the reference).  Outputs are HOST pointers: obs f64 [9], reward, valid, done.
 * By default (tg_set_serve) the call is served by a one-wave kernel resident on the device
 * (k_serve1) that polls a mailbox in pinned host memory: the call posts the action, spins on
 * the answer and returns the row the kernel wrote into pinned host memory -- no launch and no
 * synchronisation per call.  The server is launched by the first such call (after the work
 * queued on `stream`), stopped by any other call on the handle, and leaves by itself after
 * TG_SERVE_IDLE_US (default 500) microseconds without a command.  With serving off: one launch
 * on `stream` and one synchronisation of it.
 * An action outside [-9, 8] (any int32; the reference raises IndexError) is not an error of the
 * call, served or not, here and in tg_step1_py / tg_step1_pywords: it returns TG_OK with
 * valid = 0, reward = 0 and the env's current obs, runs no option and takes no draw (a caller's
 * stream state comes back as given), and sets TG_ERR_ACTION in tg_errors, as tg_step does. */
int tg_step1(tg_batch *h, int32_t action, double *obs, int32_t *reward, uint8_t *valid,
             uint8_t *done, void *stream);

/* The N = 1 calls (tg_step1, tg_step1_py, tg_reset1_py) through the resident server (on != 0,
 * the default unless TG_SERVE=0 at tg_create) or one launch + synchronisation each (0).  Stops
 * a running server.  Results are identical either way. */
int tg_set_serve(tg_batch *h, int on);

/* The N=1 drop-in drawing from a caller-held Python random stream instead of the env's own
 * (TreasureGame with the reference's module-global random, IM/:2, OB/:9): `st` (host memory)
 * is read at the call and written back with the stream advanced by exactly the draws the
 * reference's call makes, any index (odd ones too) and gauss_next included.  Served as tg_step1
 * (the resident server, or one launch and one synchronisation per call).
 *   tg_step1_py:  step(action) (TG/:91-96); outputs as tg_step1.
 *   tg_reset1_py: reset() (TG/:78-81, IM/:55-73: 2 uniform + 2 gauss), also the constructor's
 *                 build (IM/:31-53); obs f64 [9] host, may be NULL. */
int tg_step1_py(tg_batch *h, int32_t action, tg_pystate *st, double *obs, int32_t *reward,
                uint8_t *valid, uint8_t *done, void *stream);
int tg_reset1_py(tg_batch *h, tg_pystate *st, double *obs, void *stream);

/* tg_step1_py over a stream state kept elsewhere: `words` (624 uint32) and `index` (int32,
 * 0..624) are read at the call and written back advanced, in place -- for the N=1 drop-in,
 * the words and index of CPython's global random.Random object itself (Modules/_randommodule.c
 * keeps them as `int index; uint32_t state[624]`; the Python side checks the layout against
 * random.getstate() first), so a step costs no getstate / setstate.  A step draws no gauss, so
 * gauss_next is not an argument. */
int tg_step1_pywords(tg_batch *h, int32_t action, uint32_t *words, int32_t *index, double *obs,
                     int32_t *reward, uint8_t *valid, uint8_t *done, void *stream);

/* K steps in one call with the on-device synthetic policy (TG_POLICY_*): step t0 + s takes
 * the actions tg_policy_actions(action_seed, t0 + s) would give, evaluated inside the step's
 * first kernel (no action launch, no host round trip).  Outputs are step-major: actions (may
 * be NULL) int32 [K][N], obs (may be NULL) f64 [K][N][9], reward int32 [K][N], valid u8
 * [K][N], done u8 [K][N].  flags: TG_STEP_AUTORESET (episodes queue for tg_episodes).
 * Identical to K x (tg_policy_actions + tg_step).  The fused-rollout API of SURVEY §8f-3: the
 * reference has no batched or multi-step API (callers loop over TreasureGame.step, TG/:91-96). */
int tg_rollout(tg_batch *h, int32_t steps, uint64_t action_seed, int64_t t0, int policy,
               uint32_t flags, int32_t *actions, double *obs, int32_t *reward, uint8_t *valid,
               uint8_t *done, void *stream);

/* Step the batch as `groups` contiguous groups (1..16, each >= 4096 envs; 1 = off, the default)
 * in tg_rollout: each group's steps go on a stream of its own, forked from and joined back to
 * the caller's, so one group's latency-bound option loops overlap another's bandwidth-bound
 * passes.  Results are identical (the envs share nothing); counters and timing are unchanged
 * in meaning (timing samples group 0's kernels).  stagger != 0: group g + 1 starts after group
 * g's first k_classify.  Synchronises.  (No reference counterpart: batching is new.) */
int tg_set_groups(tg_batch *h, int32_t groups, int32_t stagger);

/* A step limit on episodes, applied on the device (the reference registers no TimeLimit; this is
 * gymnasium's, with the same-step reset of TG_STEP_AUTORESET).  max_steps: 0 = off (the default),
 * 1 .. 2^30 - 1; anything else is TG_E_INVAL.  Takes effect with the next step.
 *   Scope: tg_step, tg_rollout and tg_rollout_mlp, in TG_MODE_COMPACT and TG_MODE_DIRECT, with or
 *     without tg_set_groups.  tg_step in TG_MODE_FLOW too (it runs as compact); tg_rollout in
 *     TG_MODE_FLOW with a limit set returns TG_E_INVAL and changes nothing (k_flow has no step
 *     boundary to apply it at), as tg_rollout_mlp does there with or without one.  The N = 1 calls
 *     (tg_step1*, tg_reset1*, the resident server) ignore the limit.
 *   Length: after a step's kernels env i's episode length is len = tstep + 1 - (its episode's
 *     start step), in uint32 arithmetic: the value tg_read_state's ep[i][1] reports.  The env is
 *     truncated in this step iff len >= max_steps.  An env that terminated and was auto-reset in
 *     this step has len == 0, so termination wins at len == max_steps.  (>=: lowering the limit, or
 *     restoring ep lengths past it with tg_write_state, truncates at the next step.)
 *   With TG_STEP_AUTORESET a truncated env, in the same call: appends {env, ret,
 *     len | TG_EPISODE_TRUNCATED} to the episode queue (bound and dropped-record accounting as
 *     for any record); is reset exactly as tg_reset with a mask on that env would reset it (the
 *     same draws from its own stream: the reference's env.reset() right after that step()); has
 *     its obs row of this step rewritten with the new episode's first observation and its done
 *     row set to TG_DONE_TRUNCATED; final_obs, if given, already holds its pre-reset row and is
 *     not touched; tg_read_state's ep becomes (0, 0); tg_stats.episodes and .episodes_truncated count it and
 *     its reset's draws are added to .draws, as an auto-reset's are.
 *   Without the flag a truncated env only gets done |= TG_DONE_TRUNCATED: no reset, no record,
 *     and it is flagged again at every later step (gymnasium's TimeLimit).
 *   With the limit off nothing changes: the kernels launched and their arguments are the same.
 * A step with the limit on is bit for bit (states, MT streams, obs rows, later trajectories) the
 * same step with the limit off followed by tg_reset(mask = the truncated envs). */
int tg_set_time_limit(tg_batch *h, int32_t max_steps);

/* available_mask for every env: u16 [N], bit k == option k can run. */
int tg_available_mask(tg_batch *h, uint16_t *mask, void *stream);

/* available_mask of a 1-env handle (the N=1 drop-in's TreasureGame.available_mask, TG/:83-89)
 * into a HOST u16: served by the resident server like tg_step1 (so a mask read between steps
 * does not stop it), or one launch + synchronisation with serving off. */
int tg_available_mask1(tg_batch *h, uint16_t *mask, void *stream);

/* reset() of a 1-env handle on its own stream (the N=1 drop-in's TreasureGame(seed=s).reset(),
 * TG/:78-81) with the obs row into HOST memory (obs f64 [9], may be NULL): tg_reset of the one
 * env, served by the resident server like tg_step1, or one launch + synchronisation with
 * serving off. */
int tg_reset1(tg_batch *h, double *obs, void *stream);

/* current observation of every env, f64 [N][9]. */
int tg_observe(tg_batch *h, double *obs, void *stream);

/* Synthetic action stream for step t (bench / parity): see TG_POLICY_*.  g is the GLOBAL env
 * index, so trajectories are independent of how the batch is sharded. */
int tg_policy_actions(tg_batch *h, uint64_t action_seed, int64_t t, int policy, int32_t *actions,
                      void *stream);

/* Moves up to `cap` completed-episode records (oldest first) to the device buffer `out` and
 * their number (int32) to the device word `count`; the rest stay queued for the next call.
 * Asynchronous (no host sync), so it can feed a per-step RCCL gather directly. */
int tg_episodes(tg_batch *h, tg_episode *out, int32_t *count, int32_t cap, void *stream);

/* OR of all per-env error bits (host, synchronises the handle's stream). */
int tg_errors(tg_batch *h, uint32_t *or_of_flags, void *stream);

/* Step implementation (both bit-identical):
 *   TG_MODE_COMPACT (default): k_classify finishes envs whose option cannot run and appends
 *     the rest to per-option worklists; k_run's waves run them in 64-env chunks,
 *     longest-option-first (run_blocks is reserved, pass 0).
 *   TG_MODE_DIRECT: one k_step lane per env runs its option in place. */
#define TG_MODE_DIRECT 0
#define TG_MODE_COMPACT 1
/*   TG_MODE_FLOW: as TG_MODE_COMPACT for tg_step; tg_rollout runs up to 16 steps per launch of
 *     k_flow, in which each 64-env chunk is classified for step t + 1 as soon as its envs are
 *     done with step t (no batch-wide barrier between steps).  Results are
 *     identical to the other modes. */
#define TG_MODE_FLOW 2
/*   (Round 2's TG_MODE_ASYNC, all K steps of tg_rollout in one persistent launch, was exact
 *     but slower, 0.214 vs 0.142 ms per step, and was removed in round 3: DESIGN.md §9.1.) */
int tg_set_mode(tg_batch *h, int mode, int run_blocks);

/* HIP-event timing of every `every`-th step launch (tg_step, tg_rollout's launches; 0 = off):
 * three event records around a timed launch (start, after the first kernel, end), accumulated
 * into tg_stats.kernel_ms / run_ms / timed_launches.  An event record between two kernels costs
 * the stream a gap of several microseconds, so a benchmark samples (e.g. every 8th step). */
int tg_set_timing(tg_batch *h, int every);

/* Regenerate every stale MT half still queued now (k_regen).  The compact step lists the halves
 * its envs left stale and regenerates the lists of REGEN_STEPS (16) steps at once, so up to 15
 * steps' worth may be pending after a tg_step; results never depend on when this runs (a lane
 * that reaches a stale half regenerates it itself).  A timed loop calls it at its end so that it
 * contains the regeneration work of its own steps.  Asynchronous on `stream`. */
int tg_regenerate(tg_batch *h, void *stream);
/* Capacity of the completed-episode queue (default max(4N, 65536) records).  Records that
 * arrive while it is full are dropped and counted (tg_stats.episodes_dropped); the count is
 * clamped so that an undrained queue never overflows.  Reallocates the queue and discards
 * what it holds (synchronises). */
int tg_set_episode_capacity(tg_batch *h, int32_t cap);
/* The six collision predicates of _TreasureGameImpl (up_clear, can_go_up, can_go_down,
 * can_go_left, can_go_right, can_fall: _treasure_game_impl.py:232-288) evaluated BY THE DEVICE
 * at every pixel position of [x0, x1) x [y0, y1), doors closed per door_bits (bit i = door i of
 * the objects file): out u8 [(y1-y0)][(x1-x0)] (device), bit k = predicate k.  A check hook for
 * the device build of the cell-level probes against the reference's truth tables. */
int tg_predicate_table(tg_batch *h, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                       uint32_t door_bits, uint8_t *out, void *stream);
/* Counters (host, synchronises). */
int tg_get_stats(tg_batch *h, tg_stats *out);
int tg_stats_reset(tg_batch *h);
/* Resources of the step kernels as launched on this handle's device (no reference counterpart;
 * for the measurement's notes): kernel TG_KERNEL_*; out: workgroups per CU by the occupancy
 * API, VGPRs, SGPRs, static LDS bytes per 256-thread workgroup. */
#define TG_KERNEL_CLASSIFY 0 /* k_classify, uniform policy given as actions, auto-reset */
#define TG_KERNEL_RUN 1      /* k_run, auto-reset */
#define TG_KERNEL_REGEN 2    /* k_regen */
int tg_kernel_info(tg_batch *h, int kernel, int32_t *blocks_per_cu, int32_t *vgprs, int32_t *sgprs,
                   int32_t *lds_bytes);
/* Per-env MT19937 storage of this build (no reference counterpart; for sizing and for the
 * measurement's byte counts): ring_words = the word positions of the ring of pre-twisted
 * generations, stored_words = the words kept in HBM (the even generations), code_bytes = one
 * draw code per random() of the ring.  Any pointer may be NULL. */
int tg_mt_layout(int32_t *ring_words, int32_t *stored_words, int32_t *code_bytes);

/* Diagnostic (a timed region's fixed costs): `kernels` dependent launches of an
 * empty kernel of `blocks` 256-thread workgroups on `stream` (the platform's dispatch gap between
 * two dependent kernels, and an idle GPU's first dispatch).  No reference counterpart. */
int tg_probe_dispatch(int32_t kernels, int32_t blocks, void *stream);
/* Diagnostic: the device buffers, pinned host buffers, streams and events the library holds in
 * this process now, over every handle (one counter, kept where they are acquired and released).
 * It returns to its earlier value when a handle is destroyed, and when a call fails.  No
 * reference counterpart. */
int64_t tg_live_resources(void);

/* Raw SoA state copy-out for checkpoints and tests (host buffers, synchronises; the MT
 * generations are gathered on the device and copied out in chunks of 64 Ki envs):
 * pos int32 [N][2], flags u32 [N], objs int32 [N][4] (key cx,cy, gold cx,cy),
 * ang f64 [N][2], mt u32 [N][624], mt_pos u32 [N], ep int32 [N][2] (auto-reset episode
 * return, length so far).  Any pointer may be NULL.
 *
 * flags: one word per env,
 *   bits 0..4    jump_ticker (0..23)
 *   bit  5       facing_right
 *   bit  6 + i   the boolean of interactive object i, in the order doors, handles, bolt, each
 *                kind in the order of the objects file: door.closed at bits 6..8, handle.up at
 *                bits 9..10, bolt.locked at bit 11
 *   bits 12..14  len(player_bag) (0..7)
 *   bit  15 + j  item j of player_bag, j = 0 the first one picked up: 1 = the gold coin, 0 = the
 *                key; 0 for j >= len(player_bag)
 *   bits 22..23  not used, 0
 *   bits 24..31  the env's TG_ERR_* bits (sticky: a reset keeps them; 0 in a healthy env)
 * objs: the cells the reference keeps in key.cx, key.cy, goldcoin.cx, goldcoin.cy (an item in
 * the bag lies in the bottom row, a used key at (-1, -1)); each fits an int8.
 * ang: handle.angle of the level's two handles, in the order of the objects file.
 * ep: the unfinished episode of the env, as tg_episode counts a finished one: ep[i][0] is the
 * sum of the step rewards (None counts 0) and ep[i][1] the number of env-steps, valid or not,
 * since the env's last reset (tg_reset, tg_reset1 or the auto-reset of a step that returned
 * done; the constructor's state before any step: 0, 0).  A step that returns done without
 * TG_STEP_AUTORESET counts like any other, so (0, 0) holds right after a reset only.
 * (mt, mt_pos) is the env's random.getstate() equivalent: the MT19937 generation holding the
 * env's next word and the index of that word in it, always even (a random() takes two words)
 * and in 0..622.  Where CPython holds (generation, 624), "twist before the next word" -- the
 * state after the last word of a generation -- this call reports the same stream position as
 * (the twisted successor generation, 0); random.setstate() accepts either form and continues
 * identically. */
int tg_read_state(tg_batch *h, int32_t *pos, uint32_t *flags, int32_t *objs, double *ang,
                  uint32_t *mt, uint32_t *mt_pos, int32_t *ep);
/* Checkpoint restore, the inverse of tg_read_state (host buffers, synchronises): every env
 * continues bit-exactly from the given state.  All pointers but ep are required (ep NULL =
 * zeros); mt_pos must be even and in 0..624 (this path's draws consume words in pairs; 624 =
 * CPython's "twist before the next draw", the same position as the successor generation at 0),
 * i.e. any random.getstate() of the reference env reached through step()/reset(), and what
 * tg_read_state returns (0..622).  pos must fit an int16 and objs an int8 each.  ep is the
 * (return, length) pair of tg_read_state: the next finished episode of the env reports them
 * plus its steps after the restore.  A call that fails (TG_E_INVAL) has changed nothing.  The
 * episode queue and counters are not touched. */
int tg_write_state(tg_batch *h, const int32_t *pos, const uint32_t *flags, const int32_t *objs,
                   const double *ang, const uint32_t *mt, const uint32_t *mt_pos,
                   const int32_t *ep);

/* ---- device-resident snapshots: save, load and fork envs (an extension) ---------------------
 * The reference idiom is copy.deepcopy(env), optionally followed by random.seed(s): "put env j
 * into the state env i had then".  A snapshot holds `slots` saved envs in device memory; a slot
 * is tg_read_state's record of one env (2,536 B: the 16-B state word, the two angles, the
 * episode's (return, length) and the MT generation holding the position with its index), a tenth
 * of an env's ring.  tg_snap_save and tg_snap_load move envs to slots and slots to envs through
 * DEVICE index arrays of `count` entries (env indices local to the handle): they only launch
 * kernels on `stream`, allocate nothing, copy nothing to the host and never synchronise, so they
 * can be queued between rollouts; what they need is allocated by tg_snap_create.  count == 0:
 * TG_OK, nothing launched.
 *
 * A snapshot belongs to the handle that created it (same device, same level): any other handle
 * gets TG_E_INVAL.  Its buffers are counted by tg_live_resources; tg_destroy(h) frees the
 * snapshots tg_snap_destroy did not.
 *
 * tg_snap_save: slot slots[k] receives env envs[k] as it is at that point of the stream (whatever
 * ring generation it is in, and whether or not a half of its ring awaits regeneration: neither
 * shows in the slot).  The envs are not changed.
 * tg_snap_load: env envs[k] becomes slot slots[k]: its game state, its episode (the return and
 * the length so far: the next finished episode reports them plus its steps after the load, and
 * tg_set_time_limit counts the length), and its stream, which continues bit for bit as
 * tg_write_state of the same record would make it continue (index 624 included).  A slot may be
 * named any number of times (fan-out).  With seeds != NULL env envs[k] takes the slot's game
 * state and episode, and the stream of random.seed(seeds[k]) (what
 * random.Random(seeds[k]).getstate() continues): copy.deepcopy(env), then random.seed(s).
 * Envs a load does not name are untouched: state, stream, pending regeneration and its 16-step
 * cadence (tg_regenerate) are what they would be without the call.  The episode queue and
 * tg_get_stats's counters are not touched.
 * An envs[k] outside [0, N) or a slots[k] outside [0, slots) makes that entry a no-op and sets
 * TG_ERR_INDEX in what tg_errors reports (a bit of the handle, never of an env's flag word);
 * nothing is read or written out of bounds.  Two entries of one call that name the same target
 * (an env in a load, a slot in a save) leave that target unspecified and nothing else written.
 * TG_E_INVAL, with nothing launched: a null handle, snapshot, envs or slots; count < 0; a
 * snapshot of another handle; slots <= 0 in tg_snap_create.
 *
 * tg_snap_read / tg_snap_write: slots [first, first + count) out to and in from host buffers in
 * tg_read_state's and tg_write_state's formats, with tg_write_state's validation (mt_pos even and
 * 0..624, pos within int16, objs within int8; all of write's pointers but ep required, ep NULL =
 * zeros; any of read's may be NULL).  They synchronise.  A failed write has changed nothing.  A
 * written record is stored as given and read back verbatim (mt_pos 624 too; a saved one has
 * 0..622), so an archive persists across handles and runs.  A slot never written holds zeros. */
#define TG_ERR_INDEX (1u << 31)   /* tg_snap_save / tg_snap_load: an env or slot index out of range */
typedef struct tg_snap tg_snap;
int tg_snap_create(tg_batch *h, int64_t slots, tg_snap **out);   /* allocates; synchronises */
void tg_snap_destroy(tg_snap *s);                                /* also freed by tg_destroy(h) */
int64_t tg_snap_slots(const tg_snap *s);
int tg_snap_save(tg_batch *h, tg_snap *s, const int64_t *envs, const int64_t *slots, int64_t count,
                 void *stream);
int tg_snap_load(tg_batch *h, const tg_snap *s, const int64_t *slots, const int64_t *envs,
                 const uint64_t *seeds, int64_t count, void *stream);
int tg_snap_read(tg_snap *s, int64_t first, int64_t count, int32_t *pos, uint32_t *flags,
                 int32_t *objs, double *ang, uint32_t *mt, uint32_t *mt_pos, int32_t *ep);
int tg_snap_write(tg_snap *s, int64_t first, int64_t count, const int32_t *pos,
                  const uint32_t *flags, const int32_t *objs, const double *ang, const uint32_t *mt,
                  const uint32_t *mt_pos, const int32_t *ep);

/* ---- render('rgb_array') -----------------------------------------------------------------
 * Sprite sheet: TG_SPR_COUNT RGBA8 images of sprite_w x sprite_h (the reference's PNGs decoded,
 * e.g. by PIL, in this order; the reference scales each to 48x48 at load, DR/:57-134). */
#define TG_SPR_BACKGROUND 0     /* 5 variants: sprites/background/background_{0..4}.png */
#define TG_SPR_WALL 5           /* 5 variants: sprites/wall/wall_{0..4}.png */
#define TG_SPR_FLOOR 10         /* 5 variants: sprites/floor/floor-{0..4}.png */
#define TG_SPR_LADDER 15        /* sprites/ladder.png */
#define TG_SPR_DOOR_CLOSED 16   /* sprites/closeddoor.png */
#define TG_SPR_DOOR_OPEN 17     /* sprites/open-door.png */
#define TG_SPR_KEY 18           /* sprites/key.png */
#define TG_SPR_GOLD 19          /* sprites/gold.png */
#define TG_SPR_BOLT_OPEN 20     /* sprites/bolt-open.png */
#define TG_SPR_BOLT_LOCKED 21   /* sprites/bolt-locked.png */
#define TG_SPR_HERO 22          /* sprites/hero.png */
#define TG_SPR_HANDLE_BASE 23   /* sprites/handle-base.png */
#define TG_SPR_COUNT 24

/* Build the renderer's static layer and sprite tables (HOST sprite pointer; synchronises).
 * Must precede tg_render; may be called again to change the sheet. */
int tg_render_init(tg_batch *h, const uint8_t *sprites_rgba, int32_t sprite_w, int32_t sprite_h);
/* Frame size in pixels: H*48 rows x W*48 columns (624 x 672 for the default level). */
int tg_frame_shape(const tg_batch *h, int32_t *height, int32_t *width);
/* render('rgb_array') of envs [first, first+count): rgb u8 [count][height][width][3] (device,
 * 16-B aligned), the screen of each env's current state (after auto-reset, the new episode's). */
int tg_render(tg_batch *h, int64_t first, int64_t count, uint8_t *rgb, void *stream);

/* ---- downscaled / grayscale frames (an extension: the reference has no such mode) --------
 * With F the frame tg_render writes and `scale` s a divisor of 48 (1, 2, 3, 4, 6, 8, 12, 16,
 * 24, 48; anything else is TG_E_INVAL), the RGB output is the box mean with halves rounded up,
 *   out[y][x][c] = (2 * S + s*s) / (2 * s*s),  S = sum of F[s*y + dy][s*x + dx][c], dy, dx < s,
 * and the gray output is (77*R + 150*G + 29*B + 128) >> 8 of those averaged bytes.  The items
 * are composited at full resolution before the sum (the alpha blend does not commute with
 * averaging), so the result is exactly this function of tg_render's frame; scale 1 with
 * TG_FRAME_RGB is tg_render's output byte for byte.  TG_ERR_RENDER is raised as by tg_render. */
#define TG_FRAME_RGB 3
#define TG_FRAME_GRAY 1
/* Output size in pixels at `scale`: H*48/scale rows x W*48/scale columns (78 x 84 at 8). */
int tg_frame_shape_scaled(const tg_batch *h, int32_t scale, int32_t *height, int32_t *width);
/* Frames of envs [first, first+count): out u8 [count][height][width][channels] (device, 16-B
 * aligned; a frame need not be a multiple of 16 B and the frames are packed).  Needs
 * tg_render_init first (TG_E_STATE).  The first call for a scale pools the static layer and
 * the cell tiles on the host and uploads them (it synchronises); they are cached until the
 * next tg_render_init or tg_destroy (with a host copy of the static layer and sprites, about
 * 1.7 MB for the default level, that tg_render_init keeps for this).  Later calls only launch
 * on `stream`.  Because that first call allocates and copies, it cannot run inside a stream
 * capture: call each (scale) once before capturing a graph that renders at it. */
int tg_render_scaled(tg_batch *h, int64_t first, int64_t count, int32_t scale, int32_t channels,
                     uint8_t *out, void *stream);

/* ---- agent-centred windows of the frame (an extension: the reference has no such mode) -----
 * The hero's cell is the reference's get_player_cell (IM/:441-445) with floor division,
 *   xc = playerx // 48,  yc = (playery + 24) // 48.
 * For a `radius` r in 1..7 the window is the (2r+1) x (2r+1) cells with origin
 * (ox, oy) = (xc - r, yc - r) in cells and side n = 48*(2r+1) pixels.  With F the frame
 * tg_render writes,
 *   V[y][x][c] = F[48*oy + y][48*ox + x][c]  where that pixel is inside F, else 0    (y, x < n)
 * and the output is tg_render_scaled's function of V (the box mean with halves rounded up, then
 * the gray formula) for `scale` s a divisor of 48.  The origin is cell-aligned and s divides 48,
 * so every s x s box lies inside one cell of F or wholly outside F: the output equals the
 * zero-padded crop at (48*oy/s, 48*ox/s), of side n/s, of tg_render_scaled's frame (the gray of
 * black is 0); scale 1 with TG_FRAME_RGB is that crop of tg_render's frame.  r = 0 is refused:
 * the hero's 48x48 sprite at (playerx - 24, playery) spans up to 2x3 cells; for r >= 1 it lies
 * wholly inside the window.  Any position tg_write_state accepts is safe: a window partly or
 * wholly outside the frame is 0 there.  TG_ERR_RENDER is raised for every env of the range
 * exactly as by tg_render_scaled, whether or not the offending handle is in the window. */
/* Output size in pixels: both 48*(2*radius+1)/scale (18 x 18 at radius 1, scale 8). */
int tg_frame_shape_view(const tg_batch *h, int32_t radius, int32_t scale, int32_t *height,
                        int32_t *width);
/* Windows of envs [first, first+count): out u8 [count][n/s][n/s][channels] (device, packed, 16-B
 * aligned at its start; a frame may be as small as 9 B).  Nothing outside
 * [out, out + count * frame bytes) is written.  origin may be NULL; otherwise device i32
 * [count][2] = (ox, oy) in cells, where each window sits in the level.  Needs tg_render_init
 * first (TG_E_STATE); TG_E_INVAL for a radius outside 1..7, a scale that does not divide 48,
 * channels other than TG_FRAME_RGB / TG_FRAME_GRAY, a bad range or a misaligned out.  The
 * first call for a scale builds and caches that scale's pooled tables as tg_render_scaled's
 * first call does (the same cache: either call warms the other; it synchronises and cannot run
 * inside a stream capture).  Later calls only launch on `stream`. */
int tg_render_view(tg_batch *h, int64_t first, int64_t count, int32_t radius, int32_t scale,
                   int32_t channels, uint8_t *out, int32_t *origin, void *stream);

/* ---- a learned actor on the device (an extension: the reference has no policy) -------------
 * A two-hidden-layer MLP over the 9-dimensional observation with a 9-way policy head and a
 * value head.  Hidden width H is 16, 32, 64 or 128; the activation is TG_ACT_RELU or
 * TG_ACT_TANH.  The parameters are one packed f32 array of H*H + 21*H + 28 values:
 *   obs_scale[9], obs_shift[9], W1[H][9], b1[H], W2[H][H], b2[H], Wp[9][H], bp[9], Wv[H], bv[1]
 * Arithmetic: all f32, every multiply-add an explicit fmaf (the build has -ffp-contract=off).
 * With chain(c; w, x): for k ascending, c = fmaf(w[k], x[k], c), and o[9] the env's observation
 * (exactly the f64 row tg_observe writes):
 *   x[j]     = fmaf((float)o[j], obs_scale[j], obs_shift[j])
 *   a1[i]    = act(chain(b1[i]; W1[i], x))
 *   a2[i]    = act(chain(b2[i]; W2[i], a1))
 *   logit[k] = chain(bp[k]; Wp[k], a2)
 *   value    = chain(bv; Wv, a2)
 * relu is z > 0 ? z : 0, tanh is tanhf(z).  So logits and value do not depend on batch size,
 * sharding or the kernel's tiling, and a ReLU network's are reproducible bit for bit on a CPU.
 * Allowed set A: the set bits of the env's available_mask when `masked` is set and the mask is
 * non-zero, else all 9 actions (TG_POLICY_MASKED's fallback).
 * Sampling: m = max of logit[k] over A; e[k] = expf(logit[k] - m) for k in A; Z = the f32 sum of
 * e[k] over A in ascending k; h = sm64(sm64(a0 ^ sm64(g)) ^ t) with g the GLOBAL env index
 * (tg_policy_actions' hash); u = (float)(h >> 40) * 2^-24, thr = u * Z; the action is the first k
 * in A, ascending, whose running f32 sum of e exceeds thr, else the last k in A.
 * TG_MLP_GREEDY: the lowest k in A with logit[k] == m.  Both: logp = (logit[a] - m) - logf(Z).
 * With non-finite parameters or activations the results are unspecified, but every index is
 * derived from A, never from a float: nothing faults and a masked action is never chosen. */
#define TG_ACT_RELU 0
#define TG_ACT_TANH 1
#define TG_MLP_SAMPLE 0
#define TG_MLP_GREEDY 1
/* Copies the packed parameters (a DEVICE pointer) on `stream` into a buffer the handle owns,
 * device to device and asynchronously: a learner refreshes the weights between rollouts without
 * a synchronisation, and calls queued earlier on the stream still see the earlier weights.  (The
 * first load allocates that buffer.)  A bad hidden or act or a null pointer: TG_E_INVAL. */
int tg_policy_mlp_load(tg_batch *h, int32_t hidden, int32_t act, int32_t masked,
                       const float *params_dev, void *stream);
/* The actor on the current state of every env for step t: actions int32 [N], and where not NULL
 * logp f32 [N], value f32 [N], logits f32 [N][9].  mode: TG_MLP_*.  TG_E_STATE before a load. */
int tg_policy_mlp(tg_batch *h, uint64_t action_seed, int64_t t, int32_t mode, int32_t *actions,
                  float *logp, float *value, float *logits, void *stream);
/* K steps in one call with the actor as the policy: step t0 + s runs the actor kernel into row s,
 * then the step kernels with those actions given.  Step-major outputs as tg_rollout: actions
 * (may be NULL) int32 [K][N], obs (may be NULL) f64 [K][N][9], reward, valid, done, and logp,
 * value (each may be NULL) f32 [K][N].  Identical to K x (tg_policy_mlp + tg_step).  The row the
 * policy saw at step s is obs[s - 1] (for s = 0: tg_observe before the call), also after an
 * auto-reset: the row is then the new episode's first observation.  TG_MODE_COMPACT and
 * TG_MODE_DIRECT; with tg_set_groups each group launches the actor for its own envs on its own
 * stream.  TG_MODE_FLOW: TG_E_INVAL (k_flow evaluates its policy inside the kernel). */
int tg_rollout_mlp(tg_batch *h, int32_t steps, uint64_t action_seed, int64_t t0, int32_t mode,
                   uint32_t flags, int32_t *actions, double *obs, int32_t *reward, uint8_t *valid,
                   uint8_t *done, float *logp, float *value, void *stream);

/* ---- advantages on the device (an extension: the reference has no learner) -----------------
 * Generalised advantage estimation over a rollout's step-major rows, one env per column.  All
 * f32, every multiply-add an explicit fmaf, so a column's results depend on that column alone
 * (not on batch size, sharding, groups or tiling) and are reproducible bit for bit on a CPU.
 * For env i the scan runs s = K-1 .. 0 from A_K = 0, with gl = gamma * lambda (one f32 product):
 *   term  = done[s][i] & TG_DONE_TERMINATED;  trunc = done[s][i] & TG_DONE_TRUNCATED
 *   nv    = term ? 0
 *         : trunc && the env was reset in this step ? vtrunc[s][i]   (V of the pre-reset state)
 *         : s == K-1 ? vboot[i] : value[s+1][i]
 *   delta = fmaf(gamma, nv, (float)reward[s][i]) - value[s][i]
 *   carry = done[s][i] != 0 ? 0 : A_{s+1}
 *   A_s   = fmaf(gl, carry, delta)
 *   adv[s][i] = A_s;  ret[s][i] = A_s + value[s][i];  vnext[s][i] = nv
 * "Reset in this step": the rollout ran with TG_STEP_AUTORESET and a step limit.  Without the flag
 * a truncated env is not reset (tg_set_time_limit): its next state is the one value[s+1] or vboot
 * saw, so those are used and only the recursion is cut.  With auto-reset the two bits never
 * coincide (termination wins at len == max_steps); where both are set, term wins.  A step with
 * valid == 0 is an ordinary transition with reward 0; the caller masks it if it wants to.
 * vnext, "the value of the state each step led to, 0 after termination", is written in full (TD
 * targets); it is also where the truncated envs' values are handed in.
 *
 * tg_gae: the scan alone over caller-owned DEVICE rows of any rollout (a tg_step loop's too):
 * reward int32, done u8, value f32 [K][N], vboot f32 [N] in; adv, ret f32 [K][N] out.
 * vnext_given 1: vnext's entries whose done has TG_DONE_TRUNCATED set and TG_DONE_TERMINATED clear
 * are read as vtrunc before they are rewritten; 0: nothing is read from vnext, which may then be
 * NULL (not stored).  One kernel on `stream`, no synchronisation.  TG_E_INVAL, with nothing
 * launched: gamma or lambda outside [0, 1] or not finite, steps < 0, a null reward, done, value,
 * vboot, adv or ret, vnext_given with a null vnext.  steps == 0: TG_OK. */
int tg_gae(tg_batch *h, int32_t steps, float gamma, float lambda, const int32_t *reward,
           const uint8_t *done, const float *value, float *vnext, const float *vboot,
           int32_t vnext_given, float *adv, float *ret, void *stream);
/* tg_rollout_mlp, then vboot = the actor's value of every env after step K, then tg_gae.
 * Everything tg_rollout_mlp writes, and the state it leaves (MT streams, episode queue, stats),
 * is bit for bit what it is without the advantages; value is required here.  With a step limit
 * and TG_STEP_AUTORESET, each step also saves the state words of the envs the limit is about to
 * reset, before they are reset (one small kernel per step into a device-side list), and a
 * value-only actor kernel runs over the list after the last step (earlier when the list's bound
 * is reached), so the cost follows the number of truncated envs.  The values go to vnext[s][i]
 * and the scan reads those (vnext_given = 1); each is tg_policy_mlp's value of that state.
 * Otherwise vnext_given = 0.
 * vboot f32 [N] (NULL: a scratch the handle owns) is tg_policy_mlp's value row after the call.
 * With tg_set_groups the per-step kernels run on the groups' streams with lists of their own;
 * vboot and the scan follow on the caller's stream after the join.  No synchronisation (the
 * lists and the scratch are allocated at first use).
 * TG_E_INVAL, with nothing changed (the step count included): gamma or lambda outside [0, 1] or
 * not finite; a null adv, ret or value; a null vnext while a limit is set and TG_STEP_AUTORESET is
 * given (with no limit vnext may be NULL: not stored); TG_MODE_FLOW; more than 2^28 envs in the
 * handle (or in a group) with a limit and TG_STEP_AUTORESET (the list's count is an int32 over
 * 4 entries per env); whatever tg_rollout_mlp rejects.  steps == 0: TG_OK. */
int tg_rollout_mlp_gae(tg_batch *h, int32_t steps, uint64_t action_seed, int64_t t0, int32_t mode,
                       uint32_t flags, int32_t *actions, double *obs, int32_t *reward,
                       uint8_t *valid, uint8_t *done, float *logp, float *value, float gamma,
                       float lambda, float *adv, float *ret, float *vnext, float *vboot,
                       void *stream);

const char *tg_last_error(void);
const char *tg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TG_AMD_H */
