// tg_snapshot.h — one saved env (tg_snap_*, include/tg_amd.h): the slot and its codec, the gather
// of the generation holding an env's position from its ring (k_snap_save, and tg_read_state's
// k_gather_mt), and the per-lane form of the ring's rebuild from a slot (k_snap_load does it with
// a whole wave, tg_twist.h).  `__host__ __device__`; tests/native_snapshot builds it for the host.
//
// A slot is tg_read_state's record of one env, 2,536 B:
//   st4  16 B    the env's state word (tg_state.h), its MT word reduced to CPython's index into the
//                generation below (0..622 from a save; 0..624 as written by tg_snap_write),
//                MT_STALE and MT_LISTED clear
//   ang  16 B    the two handle angles
//   ep    8 B    (return so far, length so far): a length, not the start step Soa::ep keeps
//   mt 2,496 B   the generation holding the position (random.getstate()'s 624 words)
// The four fields are four arrays over the slots (Snap), so a slot's generation is 156 aligned
// uint4 and the small words are coalesced over an index list.
#pragma once
#include "tg_mt.h"

namespace tg {

constexpr int SNAP_Q = MT_N / 4;  // uint4 per generation
constexpr int SNAP_SLOT_BYTES = 16 + 16 + 8 + 4 * MT_N;
static_assert(MT_N % 4 == 0 && SNAP_SLOT_BYTES == 2536, "a slot: three small words and 156 uint4");

// the slots of one snapshot (kernel argument; device or host arrays)
struct Snap {
  uint4* st4;
  double2* ang;
  int2* ep;
  uint32_t* mt;  // [slots][MT_N]
};

// ---- the slot codec ----------------------------------------------------------------------------
// CPython's index of ring position pos: into the generation holding it
TG_HD uint32_t snap_index(uint32_t mti) { return (mti & MT_POS_MASK) % (uint32_t)MT_N; }
// ring generation holding the position
TG_HD uint32_t snap_gen(uint32_t mti) { return (mti & MT_POS_MASK) / (uint32_t)MT_N; }
// env -> slot: the state word with the index for its MT word; the episode's start step -> length
TG_HD uint4 snap_pack_st4(uint4 s) {
  s.w = snap_index(s.w);
  return s;
}
TG_HD int2 snap_pack_ep(int2 ep, uint32_t tstep) {
  ep.y = (int32_t)(tstep - (uint32_t)ep.y);
  return ep;
}
// slot -> env: the slot's generation goes to ring generation 0, so its index is the ring position
// (624: the first word of generation 1, its successor, as tg_write_state); length -> start step.
// With reseed the env takes a fresh stream at position 0 instead.
TG_HD uint4 snap_unpack_st4(uint4 s, bool reseed) {
  s.w = reseed ? 0u : (s.w & MT_POS_MASK);
  return s;
}
TG_HD int2 snap_unpack_ep(int2 ep, uint32_t tstep) {
  ep.y = (int32_t)(tstep - (uint32_t)ep.y);
  return ep;
}

// ---- the gather --------------------------------------------------------------------------------
// Words 4q .. 4q + 3 of ring generation g of an env whose stored words start at mt: an even
// generation's are stored (one 16-B load), an odd one's are twisted from the stored generation
// before it, which lies in the same half (a half starts on a stored generation) and so is never
// the stale one.
TG_HD uint4 snap_gen_quad(const uint32_t* mt, uint32_t g, int q) {
  if (g & 1u) {
    const uint32_t* const prev = mt + mt_store_off(g - 1u);
    return make_uint4(twist_at(prev, 4 * q), twist_at(prev, 4 * q + 1), twist_at(prev, 4 * q + 2),
                      twist_at(prev, 4 * q + 3));
  }
  return reinterpret_cast<const uint4*>(mt + mt_store_off(g))[q];
}
// the whole generation holding the position of state word mti (per-lane form of k_snap_save)
TG_HD void snap_gather(const uint32_t* mt, uint32_t mti, uint32_t* gen) {
  const uint32_t g = snap_gen(mti);
  for (int q = 0; q < SNAP_Q; ++q) {
    const uint4 v = snap_gen_quad(mt, g, q);
    gen[4 * q] = v.x, gen[4 * q + 1] = v.y, gen[4 * q + 2] = v.z, gen[4 * q + 3] = v.w;
  }
}

// ---- the rebuild ---------------------------------------------------------------------------------
// the two draw codes of words 4q .. 4q + 3 (draws 2q and 2q + 1 of the generation), low byte first
TG_HD uint32_t snap_quad_codes(const uint4 v) {
  return draw_code_words(v.x, v.y) | (draw_code_words(v.z, v.w) << 8);
}
// An env's ring from a slot's generation (per-lane form of k_snap_load, and what tg_write_state
// makes of the same record): the generation in ring generation 0 with its codes, then its 15
// successors, the words of the even ones and the codes of all.
TG_HD void snap_rebuild(uint32_t* mt, uint8_t* mc, const uint32_t* gen) {
  uint32_t cur[MT_N];
  for (int p = 0; p < MT_N; ++p) mt[p] = cur[p] = gen[p];
  for (int q = 0; q < SNAP_Q; ++q) {
    const uint32_t c = snap_quad_codes(make_uint4(gen[4 * q], gen[4 * q + 1], gen[4 * q + 2], gen[4 * q + 3]));
    mc[2 * q] = (uint8_t)c, mc[2 * q + 1] = (uint8_t)(c >> 8);
  }
  for (uint32_t g = 1; g < 2u * MT_HALF_GENS; ++g) {
    twist_gen_inplace(cur);
    gen_codes(cur, mc + g * (MT_N / 2));
    if (!(g & 1u))
      for (int p = 0; p < MT_N; ++p) mt[mt_store_off(g) + p] = cur[p];
  }
}

}  // namespace tg
