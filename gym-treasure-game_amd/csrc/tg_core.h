// tg_core.h — per-env Treasure Game step physics for the MI355X kernel (gfx950): the whole
// per-env core, one header per subject.
//
//   tg_state.h   constants, the flag word, `Level`, `Env`, the st4 codec, the integer helpers
//   tg_mt.h      CPython random: the MT ring, draw codes (draw_code), `Rng`, seeding
//   tg_walk.h    the plain phases' walk: walk_ticks, the multi-draw hops, the ring_* arithmetic
//   tg_map.h     the collision predicates: `Map`, `AirCells` / `AirProbe`, `LadMasks`
//   tg_rules.h   objects, `tick`, can_run, available_mask, policy_action, policy<K>, observe, resets
//   tg_option.h  one env-step: the span limits, span_loop, run_option, env_step
//
// A unit that needs less than the whole includes the narrowest of them that compiles (the
// renderer tg_state.h, the wave twist tg_mt.h, tests/native_walk tg_walk.h, the level parser
// tg_rules.h); the step kernels (tg_dev.h) and the host replay (tests/native/host_env.h) take all.
//
// Everything here is `__host__ __device__` integer code operating on one env held in
// registers.  tg_dev.h and tg_kernels.h wrap it in the batched kernels (one wavefront lane per env, level
// grid in LDS, struct-of-arrays state in HBM).  The host instantiation exists only so the
// test harness (tests/native/) can run the exact same code on the build machine, which has
// no GPU; the product API never executes it on the CPU.
//
// Differences in FORM from the reference (not in results — parity is pinned by the oracle):
//   * collision predicates (IM/:232-288) are evaluated on the 48x48-cell grid with a handful
//     of branch-free cell lookups instead of up to 104 pixel probes: the reference pixel map
//     is constant per cell (build_map IM/:204-216, door.update_map OB/:246-253) and OOB is
//     WALL (IM/:218-225) — here a 2-cell WALL border around the grid plus clamping;
//   * near_enough (OB/:46-53) is the exact integer test d^2 < r^2 (inputs are integers);
//   * the trigger cascade (OB/:76-94) is an explicit 8-bit-frame stack in one u64 register;
//   * MT19937 keeps two pre-twisted generations per env; consumption only reads (Rng); the
//     option loops read one code byte per draw (its noisy / jump / flip outcomes, draw_code)
//     instead of the double;
//   * each option's policy/tick loop is specialised at compile time to the primitive actions
//     that option can issue (a wave runs one option in the compacted kernel).
// Prefixes: TG/ treasure_game.py, IM/ _treasure_game_impl.py, OB/ _objects.py,
// MO/ _move_options.py, OP/ _option.py under gym_treasure_game/envs/.
#pragma once
#include "tg_state.h"
#include "tg_mt.h"
#include "tg_walk.h"
#include "tg_map.h"
#include "tg_rules.h"
#include "tg_option.h"
