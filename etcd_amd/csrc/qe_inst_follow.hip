// qe_inst_follow.hip — the follower kernel's instantiations (qe_follow.hpp):
// one per run-capacity bucket (log_runs <= 4, <= 8, <= 16), each with and
// without entries.  The kernel does not depend on the slot count, so this
// object is compiled once, not per QE_S.
#include "qe_follow.hpp"

namespace qe {

namespace {
template <int RM>
int launch_follow(const FArgs &a, dim3 grid, hipStream_t st) {
  if (a.E)
    hipLaunchKernelGGL((k_follow<RM, true>), grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((k_follow<RM, false>), grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}
}  // namespace

// One tile per wave (qe_launch.hpp tile_grid).
int dispatch_follow(const FArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.G, num_cus(), a.stats != nullptr));
  if (a.R <= 4) return launch_follow<4>(a, grid, st);
  if (a.R <= 8) return launch_follow<8>(a, grid, st);
  return launch_follow<16>(a, grid, st);
}

}  // namespace qe
