// qe_inst_vote.hip — the vote kernel's instantiations (qe_vote.hpp): the two
// mask types, each with and without the Votes rows (a voter-only launch).  The
// kernel takes the slot count at run time, so this object is compiled once,
// not per QE_S.
#include "qe_vote.hpp"

namespace qe {

namespace {
template <typename MT>
int launch_vote(const VArgs &a, dim3 grid, hipStream_t st) {
  if (a.voted)
    hipLaunchKernelGGL((k_vote<MT, true>), grid, dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((k_vote<MT, false>), grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}
}  // namespace

// One tile per wave (qe_launch.hpp tile_grid).
int dispatch_vote(const VArgs &a, hipStream_t st) {
  const dim3 grid(tile_grid(a.G, num_cus(), a.stats != nullptr));
  if (a.S <= 8) return launch_vote<uint8_t>(a, grid, st);
  return launch_vote<uint16_t>(a, grid, st);
}

}  // namespace qe
