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

// One tile per wave (as qe_tick).  With statistics the grid is capped and the
// waves walk: every wave ends with one atomic per counter.
int dispatch_follow(const FArgs &a, hipStream_t st) {
  const uint64_t tiles = (a.G + 63) / 64;
  uint64_t blocks = (tiles + (kBlock / 64) - 1) / (kBlock / 64);
  const uint64_t cap = a.stats ? static_cast<uint64_t>(num_cus()) * 8 : 0x7FFFFFFFull;
  if (blocks > cap) blocks = cap;
  const dim3 grid(static_cast<unsigned>(blocks ? blocks : 1));
  if (a.R <= 4) return launch_follow<4>(a, grid, st);
  if (a.R <= 8) return launch_follow<8>(a, grid, st);
  return launch_follow<16>(a, grid, st);
}

}  // namespace qe
