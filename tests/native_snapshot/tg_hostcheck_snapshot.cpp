// tg_hostcheck_snapshot.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the snapshot slot's code (gym-treasure-game_amd/csrc/tg_snapshot.h): the
// slot codec, the gather of the generation holding an env's position from its ring, and the
// per-lane rebuild of a ring from a slot — the functions k_snap_save and k_snap_load restate per
// lane and per wave — over one env's ring in host memory, so tests/test_snapshot_host.py can hold
// them to CPython's random and to tests/state_codec.py.  The product library never contains or
// calls this.  With HS_MAIN: a stand-alone program that runs the same functions (tests/
// native_snapshot/Makefile `asan`).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gym-treasure-game_amd/csrc/tg_snapshot.h"

extern "C" {

int hs_ring_words(void) { return tg::MT_STORE; }
int hs_ring_codes(void) { return tg::MT_CODES; }
int hs_slot_bytes(void) { return tg::SNAP_SLOT_BYTES; }

// random.seed(seed) into a ring: mt [MT_STORE], mc [MT_CODES]; the state word is 0
void hs_init(uint64_t seed, uint32_t* mt, uint8_t* mc) {
  uint32_t gen[tg::MT_N];
  tg::genrand_prefix(gen);
  tg::init_mt(mt, gen, seed, mc);
}

// `count` random() from the ring at state word *state (tg::Rng: halves left behind are stale, a
// stale one entered is regenerated first); out (may be null) takes the doubles' bits
void hs_draw(uint32_t* mt, uint8_t* mc, uint32_t* state, int64_t count, uint64_t* out) {
  tg::Rng rng(mt, *state, mc);
  for (int64_t k = 0; k < count; ++k) {
    const double r = rng.random();
    if (out) memcpy(out + k, &r, sizeof r);
  }
  *state = rng.finish();
}

// the slot's MT part of an env: the generation holding the position, and CPython's index
uint32_t hs_gather(const uint32_t* mt, uint32_t state, uint32_t* gen) {
  tg::snap_gather(mt, state, gen);
  return tg::snap_index(state);
}

// a ring (mt, mc) from a slot's generation
void hs_rebuild(uint32_t* mt, uint8_t* mc, const uint32_t* gen) { tg::snap_rebuild(mt, mc, gen); }

// the st4 codec and the slot codec on one record.  env -> slot (save) of an env whose state word
// holds (pos, flags, objs, mti) and whose episode is (ret, start step) at handle step tstep:
// slot_st4 [4], slot_ep [2]
void hs_save(const int32_t* pos, uint32_t flags, const int32_t* objs, uint32_t mti, const int32_t* ep,
             uint32_t tstep, uint32_t* slot_st4, int32_t* slot_ep) {
  tg::Env e{};
  e.px = pos[0], e.py = pos[1], e.f = flags;
  e.kx = objs[0], e.ky = objs[1], e.gx = objs[2], e.gy = objs[3];
  e.mti = mti;
  const uint4 s = tg::snap_pack_st4(tg::pack(e));
  slot_st4[0] = s.x, slot_st4[1] = s.y, slot_st4[2] = s.z, slot_st4[3] = s.w;
  const int2 p = tg::snap_pack_ep(make_int2(ep[0], ep[1]), tstep);
  slot_ep[0] = p.x, slot_ep[1] = p.y;
}
// slot -> env (load) at handle step tstep: the record's fields, the env's MT word and its
// (ret, start step)
void hs_load(const uint32_t* slot_st4, const int32_t* slot_ep, uint32_t tstep, int reseed, int32_t* pos,
             uint32_t* flags, int32_t* objs, uint32_t* mti, int32_t* ep) {
  const uint4 s = tg::snap_unpack_st4(make_uint4(slot_st4[0], slot_st4[1], slot_st4[2], slot_st4[3]),
                                      reseed != 0);
  tg::Env e;
  tg::unpack_st4(s, e);
  pos[0] = e.px, pos[1] = e.py, *flags = e.f;
  objs[0] = e.kx, objs[1] = e.ky, objs[2] = e.gx, objs[3] = e.gy;
  *mti = e.mti;
  const int2 p = tg::snap_unpack_ep(make_int2(slot_ep[0], slot_ep[1]), tstep);
  ep[0] = p.x, ep[1] = p.y;
}

}  // extern "C"

#ifdef HS_MAIN
// every generation of a ring gathered and rebuilt, the rebuilt ring continued and compared with
// the original's continuation (heap buffers of the exact sizes: the sanitizer sees every access)
int main() {
  int bad = 0;
  for (int g = 0; g < 2 * tg::MT_HALF_GENS + 3; ++g) {
    std::vector<uint32_t> mt(tg::MT_STORE), mt2(tg::MT_STORE), gen(tg::MT_N);
    std::vector<uint8_t> mc(tg::MT_CODES), mc2(tg::MT_CODES);
    hs_init(1234u + (uint64_t)g, mt.data(), mc.data());
    uint32_t state = 0;
    hs_draw(mt.data(), mc.data(), &state, (int64_t)g * (tg::MT_N / 2) + (g % 3 == 0 ? 0 : g % 3 == 1 ? 1 : 311),
            nullptr);
    uint32_t state2 = hs_gather(mt.data(), state, gen.data());
    hs_rebuild(mt2.data(), mc2.data(), gen.data());
    std::vector<uint64_t> a(2000), b(2000);
    hs_draw(mt.data(), mc.data(), &state, 2000, a.data());
    hs_draw(mt2.data(), mc2.data(), &state2, 2000, b.data());
    if (a != b) ++bad, printf("generation %d: the rebuilt ring's stream differs\n", g);
  }
  int32_t pos[2] = {-5, 300}, objs[4] = {-1, -1, 7, 12}, ep[2] = {-3, 90}, sep[2], lep[2], lpos[2], lobjs[4];
  uint32_t st[4], f, mti;
  hs_save(pos, 0x1234u, objs, (5u * tg::MT_N + 622u) | tg::MT_STALE | tg::MT_LISTED, ep, 100u, st, sep);
  hs_load(st, sep, 4000000000u, 0, lpos, &f, lobjs, &mti, lep);
  if (st[3] != 622u || sep[1] != 10 || mti != 622u || (uint32_t)lep[1] != 4000000000u - 10u ||
      memcmp(pos, lpos, sizeof pos) || memcmp(objs, lobjs, sizeof objs) || f != 0x1234u)
    ++bad, printf("the slot codec does not round-trip\n");
  printf("%s\n", bad ? "FAILED" : "ok");
  return bad != 0;
}
#endif
