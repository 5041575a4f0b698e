// tg_flow.hip — k_flow's own translation unit (tg_flow.h: TG_MODE_FLOW's one-launch rollout).
//
// Built with `-mllvm -disable-machine-licm` (gym_treasure_game_amd/build.py, FLOW_FLAGS): in
// tg_amd.hip's unit MachineLICM hoisted loop-invariant values out of k_flow's work loop and kept
// them live across it (123-182 VGPRs, 2-3 waves per SIMD); without the pass 121-129, 4 waves
// (DESIGN.md §9.2).  The pass stays on for every other kernel.  The device helpers k_flow shares
// with the per-step kernels are tg_dev.h's; this unit exports the launcher of the k_flow
// instantiations (tg_amd.hip's launch_flow) and their handles (the occupancy query).
#include "tg_dev.h"
#include "tg_flow.h"

namespace tg {
const void* flow_kernel(bool ar, int pol) {
  if (ar) return pol ? reinterpret_cast<const void*>(k_flow<true, 1>)
                     : reinterpret_cast<const void*>(k_flow<true, 0>);
  return pol ? reinterpret_cast<const void*>(k_flow<false, 1>)
             : reinterpret_cast<const void*>(k_flow<false, 0>);
}

template <bool AR, int POL>
static void launch(unsigned grid, hipStream_t st, const FlowArgs& a) {
  hipLaunchKernelGGL((k_flow<AR, POL>), dim3(grid), dim3(BLOCK), 0, st, a.S, a.n, a.L, a.grid, a.io,
                     a.eq, a.f, a.g0, a.stats, a.nstat, a.err, a.ks);
}
int flow_launch_args(bool ar, int pol, unsigned grid, hipStream_t st, const void* args, size_t bytes) {
  if (bytes != sizeof(FlowArgs)) return fail(TG_E_HIP, "k_flow: the units disagree on its arguments");
  const FlowArgs& a = *static_cast<const FlowArgs*>(args);
  if (ar) pol ? launch<true, 1>(grid, st, a) : launch<true, 0>(grid, st, a);
  else pol ? launch<false, 1>(grid, st, a) : launch<false, 0>(grid, st, a);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}
}  // namespace tg
