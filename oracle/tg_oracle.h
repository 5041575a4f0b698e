/* tg_oracle.h — CPU restatement of the reference Treasure Game step path.
 *
 * TEST INFRASTRUCTURE ONLY.  This is the parity oracle: only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it, and only as the checker / CPU baseline.  The
 * product path (gym-treasure-game_amd/, libtg_amd.so) never links or calls it.
 *
 * Pinned against golden vectors generated from the unmodified reference in the build
 * container (tests/golden/make_golden.py): CPython MT19937 KATs, full trajectories (uniform,
 * masked, auto-reset), 4096-env rolling hashes and 10k reset states.
 */
#ifndef TG_ORACLE_H
#define TG_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tgo_level tgo_level;
typedef struct tgo_env tgo_env;

/* --- CPython `random` restatement (F1 KATs) ------------------------------------------- */
void tgo_rng_words(uint64_t seed, int n, uint32_t *out);     /* getrandbits(32) x n        */
void tgo_rng_random(uint64_t seed, int n, double *out);      /* random() x n               */
void tgo_rng_uniform5(uint64_t seed, double *out);           /* the 5 uniform() KAT calls  */
void tgo_rng_gauss(uint64_t seed, int pairs, double *out);   /* gauss(0,2), gauss(0,48/36) */

/* --- level ------------------------------------------------------------------------------ */
tgo_level *tgo_level_parse(const char *domain, const char *objects, const char *interactions);
void tgo_level_free(tgo_level *lv);

/* --- single env (reference semantics; env == random.seed(seed); TreasureGame(); reset()) - */
size_t tgo_env_size(void);
tgo_env *tgo_env_new(const tgo_level *lv, uint64_t seed, double obs[9]);
void tgo_env_free(tgo_env *e);
/* step(a): returns 0, or -1 for an out-of-range action (the reference raises IndexError).
 * Python list indexing: a in [-9, -1] wraps. */
int tgo_step(tgo_env *e, int action, double obs[9], int32_t *reward, uint8_t *valid,
             uint8_t *done);
void tgo_reset(tgo_env *e, double obs[9]);
unsigned tgo_mask(tgo_env *e);
uint64_t tgo_draws(const tgo_env *e);
int64_t tgo_ticks(const tgo_env *e);
/* internal state: px, py, jump_ticker, doors, handles, bolt, key cx, cy, gold cx, cy,
 * facing_right, total_actions (same columns as the golden `internal` arrays) */
void tgo_internal(const tgo_env *e, int32_t out[12]);
/* the 6 collision predicates of IM/:232-288 at an arbitrary pixel position / door state
 * (bit order: up_clear, can_go_up, can_go_down, can_go_left, can_go_right, can_fall) */
unsigned tgo_predicates(tgo_env *e, int px, int py, unsigned door_bits);
/* the same over the pixel box [x0,x1) x [y0,y1), row-major u8 */
void tgo_predicate_table(tgo_env *e, int x0, int x1, int y0, int y1, unsigned door_bits,
                         uint8_t *out);

/* --- state injection (the checkpoint format of include/tg_amd.h, at tg_read_state) --------- */
/* The env continues from the given state: pos playerx, playery; flags the format's flag word
 * (jump_ticker, facing_right, the door / handle / bolt booleans, the bag; its unused and error
 * bits must be 0); objs key cx, cy, gold cx, cy; ang the handle angles in objects-file order;
 * (mt, mt_pos) random.getstate()'s words and index, 0..624 (mt NULL: the stream stays as it
 * is).  gauss_next is cleared, the options hold no target, total_actions and the draw and
 * tick counters go on.  The level must have at most 3 doors, 2 handles and 1 bolt, and a key
 * and a gold coin.  Returns 0, or -1 for a state the format does not admit. */
int tgo_env_set_state(tgo_env *e, const int32_t pos[2], uint32_t flags, const int32_t objs[4],
                      const double ang[2], const uint32_t mt[624], uint32_t mt_pos);
/* The inverse (any pointer may be NULL).  mt_pos is CPython's own index, 1..624: where the
 * product reports (successor generation, 0) this reports (generation, 624).  Returns -1 for
 * a state the format cannot hold (a bag of more than 7, a pending gauss_next). */
int tgo_env_get_state(const tgo_env *e, int32_t pos[2], uint32_t *flags, int32_t objs[4],
                      double ang[2], uint32_t mt[624], uint32_t *mt_pos);
/* tgo_step with a tick limit (cap <= 0: none): an option that has taken `cap` ticks stops
 * there, finished or not, as the product's TICK_CAP does.  Returns 1 then (the outputs and the
 * env hold the state after those ticks), else what tgo_step returns. */
int tgo_step_cap(tgo_env *e, int action, int64_t cap, double obs[9], int32_t *reward,
                 uint8_t *valid, uint8_t *done);
/* One step from each of n given states (arrays of the fields above, case-major), on at most
 * 16 threads: mask[i] = available_mask of state i, then step(actions[i]) under the tick limit
 * `cap`: obs [n][9], reward / valid / done [n], the state after (pos2 .. mt_pos2), the ticks
 * and random() draws the step took, capped[i] = 1 where it hit the limit.  actions NULL: the
 * masks only (mt may be NULL then).  Any output may be NULL.  Returns 0 or -1. */
int tgo_step_states(const tgo_level *lv, int64_t n, const int32_t *pos, const uint32_t *flags,
                    const int32_t *objs, const double *ang, const uint32_t *mt,
                    const uint32_t *mt_pos, const int32_t *actions, int64_t cap, double *obs,
                    int32_t *reward, uint8_t *valid, uint8_t *done, uint16_t *mask,
                    int32_t *pos2, uint32_t *flags2, int32_t *objs2, double *ang2, uint32_t *mt2,
                    uint32_t *mt_pos2, int64_t *ticks, int64_t *draws, uint8_t *capped,
                    int nthreads);
/* getstate() of random.Random(seed_base + i) for i in [i0, i0 + n), advanced by 312, 1, 155,
 * 156, 310, 311, 312 calls of random() for i % 7 = 0..6: index 624, 2, 310, 312, 620, 622,
 * 624; i % 7 == 0 is given in the successor form (the twisted generation, index 0).
 * mt [n][624], mt_pos [n]. */
void tgo_stream_states(uint64_t seed_base, int64_t i0, int64_t n, uint32_t *mt, uint32_t *mt_pos,
                       int nthreads);

/* --- batched driver (the CPU baseline and the parity generator) ------------------------- */
/* Runs envs g in [g0, g0+n), env g seeded seed_base+g, for `steps` env-steps with the
 * counter-hash action stream (policy 0 = uniform over 0..8, 1 = masked-uniform).
 * Any output pointer may be NULL.  Layouts are env-major: obs [n][steps+1][9] (t=0 is the
 * reset obs), reward/valid/done [n][steps+1], final_obs [n][steps+1][9] (pre-reset obs of
 * an auto-reset step, else == obs), hash/draws/ticks [n].  Returns 0 or -1. */
int tgo_run(const tgo_level *lv, uint64_t seed_base, int64_t g0, int64_t n, int steps,
            uint64_t action_seed, int policy, int autoreset, double *obs, int32_t *reward,
            uint8_t *valid, uint8_t *done, double *final_obs, uint64_t *hash, int64_t *draws,
            int64_t *ticks, int nthreads);

/* action stream + record hash shared with tests/golden/make_golden.py and the device code */
int tgo_run_episodes(const tgo_level *lv, uint64_t seed_base, int64_t g0, int64_t n, int steps,
                     uint64_t action_seed, int policy, int t_from, int64_t *count,
                     uint64_t *digest, int nthreads);
uint64_t tgo_sm64(uint64_t x);
uint64_t tgo_action_hash(uint64_t a0, uint64_t g, uint64_t t);
int tgo_pick_action(uint64_t a0, uint64_t g, uint64_t t, int masked, unsigned mask);
uint64_t tgo_rec_hash(uint64_t h, const double obs[9], int32_t reward, int valid, int done);

/* --- renderer (TG/:98-105 render('rgb_array') -> DR/ draw_domain); PARITY UNPINNED -------- */
/* sprites_rgba: TGO_SPR_COUNT (24) RGBA8 images of sw x sh in include/tg_amd.h TG_SPR_* order.
 * rgb: [H*48][W*48][3].  Returns 0, 1 (libm watch: a handle end point within 1e-9 of an
 * integer) or -1 (a handle shaft leaving the surface: unsupported). */
int tgo_render(const tgo_env *e, const uint8_t *sprites_rgba, int sw, int sh, uint8_t *rgb);
int tgo_run_render(const tgo_level *lv, uint64_t seed_base, const int64_t *envs, int64_t n,
                   int steps, uint64_t action_seed, int policy, int autoreset,
                   const uint8_t *sprites_rgba, int sw, int sh, uint8_t *frames, int nthreads);
/* Frames of n given states (the arrays of tgo_step_states; no stream is needed), on at most 16
 * threads: tgo_env_set_state, then tgo_render, per state.  frames [n][H*48][W*48][3].  Returns
 * the OR of the tgo_render codes (0 or 1), or -1 on any failure. */
int tgo_render_states(const tgo_level *lv, int64_t n, const int32_t *pos, const uint32_t *flags,
                      const int32_t *objs, const double *ang, const uint8_t *sprites_rgba, int sw,
                      int sh, uint8_t *frames, int nthreads);
/* Random(seed).choice over a sequence of length n, `count` times (DR/:83-86) */
void tgo_choice_seq(uint64_t seed, int n, int count, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
