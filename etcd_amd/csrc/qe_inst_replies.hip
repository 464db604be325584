// qe_inst_replies.hip — the replies kernels' instantiations (qe_replies.hpp):
// k_replies_count and k_replies_fill per mask width.  Neither depends on the
// slot count at compile time, so this object is compiled once, not per QE_S.
#include "qe_replies.hpp"

namespace qe {

// One block per chunk; qe_replies has checked that the chunks fit a launch.
int dispatch_replies_count(const RPArgs &a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(a.nb));
  if (a.wide)
    hipLaunchKernelGGL(k_replies_count<true>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_replies_count<false>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

int dispatch_replies_fill(const RPArgs &a, hipStream_t st) {
  const dim3 grid(list_fill_grid(a.nb, num_cus(), a.stats != nullptr));
  if (a.wide)
    hipLaunchKernelGGL(k_replies_fill<true>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_replies_fill<false>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
