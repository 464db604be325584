// qe_inst_outbox.hip — the outbox kernels' instantiations (qe_outbox.hpp):
// k_outbox_count per mask width, k_outbox_fill per run-capacity bucket (log_runs <= 4,
// <= 8, <= 16) and per message run capacity (msg_runs 0..QE_MAX_MSG_RUNS).
// Neither depends on the slot count at compile time, so this object is compiled
// once, not per QE_S.
#include "qe_outbox.hpp"

namespace qe {

// One block per chunk; qe_outbox has checked that the chunks fit a launch.
int dispatch_outbox_count(const OBArgs &a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(a.nb));
  if (a.wide)
    hipLaunchKernelGGL(k_outbox_count<true>, grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_outbox_count<false>, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int RM>
static void launch_fill(const OBArgs &a, uint32_t msg_runs, dim3 grid, hipStream_t st) {
  static_assert(QE_MAX_MSG_RUNS == 4, "one case per message run capacity");
  switch (msg_runs) {
    case 0: hipLaunchKernelGGL((k_outbox_fill<RM, 0>), grid, dim3(kBlock), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_outbox_fill<RM, 1>), grid, dim3(kBlock), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_outbox_fill<RM, 2>), grid, dim3(kBlock), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_outbox_fill<RM, 3>), grid, dim3(kBlock), 0, st, a); break;
    default: hipLaunchKernelGGL((k_outbox_fill<RM, 4>), grid, dim3(kBlock), 0, st, a); break;
  }
}

// One block per chunk; with statistics the grid is capped at 8 blocks per CU
// and the blocks walk, since every wave ends with one atomic per counter.
int dispatch_outbox_fill(const OBArgs &a, uint32_t msg_runs, hipStream_t st) {
  const uint64_t cap = a.stats ? static_cast<uint64_t>(num_cus()) * 8 : a.nb;
  const dim3 grid(static_cast<unsigned>(a.nb < cap ? a.nb : cap));
  if (a.R <= 4)
    launch_fill<4>(a, msg_runs, grid, st);
  else if (a.R <= 8)
    launch_fill<8>(a, msg_runs, grid, st);
  else
    launch_fill<16>(a, msg_runs, grid, st);
  return hip_status(hipGetLastError());
}

}  // namespace qe
