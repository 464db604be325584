// qe_inst_snap.hip — the snapshot kernels' instantiations (qe_snap.hpp):
// k_compact per run-capacity bucket (log_runs <= 4, <= 8, <= 16), k_snap per
// mask type.  Neither depends on the slot count at compile time, so this object
// is compiled once, not per QE_S.
#include "qe_snap.hpp"

namespace qe {

// One tile per wave (qe_launch.hpp tile_grid).
int dispatch_compact(const CPArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.G, num_cus(), a.stats != nullptr));
  if (a.R <= 4)
    hipLaunchKernelGGL(k_compact<4>, grid, dim3(kBlock), 0, st, a);
  else if (a.R <= 8)
    hipLaunchKernelGGL(k_compact<8>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_compact<16>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

int dispatch_snap(const SNArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.G, num_cus(), a.stats != nullptr));
  if (a.S <= 8)
    hipLaunchKernelGGL(k_snap<uint8_t>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_snap<uint16_t>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
