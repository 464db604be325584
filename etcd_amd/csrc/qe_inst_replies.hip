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

// One block per chunk; with statistics the grid is capped at 8 blocks per CU
// and the blocks walk, since every wave ends with one atomic per counter.
int dispatch_replies_fill(const RPArgs &a, hipStream_t st) {
  const uint64_t cap = a.stats ? static_cast<uint64_t>(num_cus()) * 8 : a.nb;
  const dim3 grid(static_cast<unsigned>(a.nb < cap ? a.nb : cap));
  if (a.wide)
    hipLaunchKernelGGL(k_replies_fill<true>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_replies_fill<false>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
