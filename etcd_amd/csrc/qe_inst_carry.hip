// qe_inst_carry.hip — qe_carry's kernels (qe_carry.hpp): the classify pass, the
// count over its count bytes and the fill of the local list.  The positions of
// the remote records are the routing layer's fill (qe_inst_route.hip).  None
// depends on the slot count at compile time: one object, not one per QE_S.
#define QE_ROUTE_KERNELS
#include "qe_carry.hpp"

namespace qe {

// A wave per 64-record tile of the source's capacity; with statistics the grid
// is capped and the waves walk, since every wave ends with one atomic per counter.
int dispatch_carry_classify(const CRArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_carry_classify, dim3(tile_grid(a.G, num_cus(), a.stats)), dim3(kBlock), 0,
                     st, a);
  return hip_status(hipGetLastError());
}

// A block per 4096-record chunk (the caller has checked that the chunks fit a launch).
int dispatch_carry_count(const CRArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_carry_count, dim3(static_cast<unsigned>(a.nb)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

int dispatch_carry_fill(const CRArgs &a, hipStream_t st) {
  CRArgs f = a;
  f.stats = nullptr;  // the classify pass holds the statistics
  hipLaunchKernelGGL(k_carry_fill, dim3(list_fill_grid(a.nb, num_cus(), false)), dim3(kBlock), 0,
                     st, f);
  return hip_status(hipGetLastError());
}

}  // namespace qe
