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

int dispatch_outbox_fill(const OBArgs &a, uint32_t msg_runs, hipStream_t st) {
  const dim3 grid(list_fill_grid(a.nb, num_cus(), a.stats != nullptr));
  return with_run_bucket(a.R, [&](auto rm) {
    return with_msg_runs(msg_runs, [&](auto e) {
      hipLaunchKernelGGL((k_outbox_fill<rm(), e()>), grid, dim3(kBlock), 0, st, a);
      return hip_status(hipGetLastError());
    });
  });
}

}  // namespace qe
