// qe_inst_route.hip — the routing calls' kernels (qe_route.hpp, qe_inbox.hpp,
// qe_requests.hpp): per call the init pass, the key passes and the routing pass
// (qe_inbox's per message run capacity), the fill of qe_requests's output list
// and the positions fill both deferred lists share.  None depends on the slot
// count at compile time: one object, not one per QE_S.
#define QE_ROUTE_KERNELS
#define QE_ROUTE_POSITIONS_KERNEL
#include "qe_inbox.hpp"
#include "qe_requests.hpp"

namespace qe {

// The init passes: a thread per group.  The key passes and the routing pass: a
// wave per 64-record tile; with statistics the routing pass's grid is capped
// and its waves walk, since every wave ends with one atomic per counter.
int dispatch_inbox_init(const IBArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_inbox_init, dim3(tile_grid(a.G, num_cus(), false)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

int dispatch_inbox_passes(const IBArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.n, num_cus(), false)), capped(tile_grid(a.n, num_cus(), a.stats));
  hipLaunchKernelGGL(k_inbox_p1, grid, dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(k_inbox_p2, grid, dim3(kBlock), 0, st, a);
  return with_msg_runs(a.E, [&](auto e) {
    hipLaunchKernelGGL(k_inbox_p3<e()>, capped, dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

int dispatch_requests_init(const RQArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_requests_init, dim3(tile_grid(a.G, num_cus(), false)), dim3(kBlock), 0, st,
                     a);
  return hip_status(hipGetLastError());
}

int dispatch_requests_passes(const RQArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.n, num_cus(), false)), capped(tile_grid(a.n, num_cus(), a.stats));
  hipLaunchKernelGGL(k_requests_stop, grid, dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(k_requests_route, capped, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// A block per 4096-record chunk (the caller has checked that the chunks fit a launch).
int dispatch_requests_out(const RQList &a, hipStream_t st) {
  hipLaunchKernelGGL(k_requests_out, dim3(list_fill_grid(a.nb, num_cus(), false)), dim3(kBlock), 0,
                     st, a);
  return hip_status(hipGetLastError());
}

int dispatch_route_positions(const RoutePos &a, hipStream_t st) {
  hipLaunchKernelGGL(k_route_positions, dim3(list_fill_grid(a.nb, num_cus(), false)), dim3(kBlock),
                     0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
