// qe_inst_inbox.hip — the inbox kernels' instantiations (qe_inbox.hpp): the
// init pass, the two key passes, the routing pass per message run capacity
// (msg_runs 0..QE_MAX_MSG_RUNS) and the scatter of the deferred positions.
// None depends on the slot count at compile time: one object, not one per QE_S.
#define QE_INBOX_KERNELS
#include "qe_inbox.hpp"

namespace qe {

// A thread per group.
int dispatch_inbox_init(const IBArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_inbox_init, dim3(tile_grid(a.G, num_cus(), false)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// A wave per 64-record tile; with statistics the routing pass's grid is capped
// and its waves walk, since every wave ends with one atomic per counter.
int dispatch_inbox_passes(const IBArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.n, num_cus(), false)), capped(tile_grid(a.n, num_cus(), a.stats));
  hipLaunchKernelGGL(k_inbox_p1, grid, dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(k_inbox_p2, grid, dim3(kBlock), 0, st, a);
  static_assert(QE_MAX_MSG_RUNS == 4, "one case per message run capacity");
  switch (a.E) {
    case 0: hipLaunchKernelGGL(k_inbox_p3<0>, capped, dim3(kBlock), 0, st, a); break;
    case 1: hipLaunchKernelGGL(k_inbox_p3<1>, capped, dim3(kBlock), 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_inbox_p3<2>, capped, dim3(kBlock), 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_inbox_p3<3>, capped, dim3(kBlock), 0, st, a); break;
    default: hipLaunchKernelGGL(k_inbox_p3<4>, capped, dim3(kBlock), 0, st, a); break;
  }
  return hip_status(hipGetLastError());
}

// A block per 4096-record chunk (qe_inbox has checked that the chunks fit a launch).
int dispatch_inbox_deferred(const IBArgs &a, uint64_t nb, hipStream_t st) {
  hipLaunchKernelGGL(k_inbox_deferred, dim3(static_cast<unsigned>(nb)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
