// qe_inst_requests.hip — the request kernels' instantiations (qe_requests.hpp):
// the init pass, the key pass, the routing pass and the two fills of the
// record-list layer.  None depends on the slot count at compile time: one
// object, not one per QE_S.
#define QE_REQUESTS_KERNELS
#include "qe_requests.hpp"

namespace qe {

// A thread per group.
int dispatch_requests_init(const RQArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_requests_init, dim3(tile_grid(a.G, num_cus(), false)), dim3(kBlock), 0, st,
                     a);
  return hip_status(hipGetLastError());
}

// A wave per 64-record tile; with statistics the routing pass's grid is capped
// and its waves walk, since every wave ends with one atomic per counter.
int dispatch_requests_passes(const RQArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.n, num_cus(), false)), capped(tile_grid(a.n, num_cus(), a.stats));
  hipLaunchKernelGGL(k_requests_stop, grid, dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(k_requests_route, capped, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// A block per 4096-record chunk (qe_requests has checked that the chunks fit a launch).
int dispatch_requests_out(const RQList &a, hipStream_t st) {
  hipLaunchKernelGGL(k_requests_out, dim3(list_fill_grid(a.nb, num_cus(), false)), dim3(kBlock), 0,
                     st, a);
  return hip_status(hipGetLastError());
}

int dispatch_requests_deferred(const RQList &a, hipStream_t st) {
  hipLaunchKernelGGL(k_requests_deferred, dim3(list_fill_grid(a.nb, num_cus(), false)),
                     dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
