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

// One tile per wave (as qe_tick).  With statistics the grid is capped and the
// waves walk: every wave ends with one atomic per counter.
int dispatch_vote(const VArgs &a, hipStream_t st) {
  const uint64_t tiles = (a.G + 63) / 64;
  uint64_t blocks = (tiles + (kBlock / 64) - 1) / (kBlock / 64);
  const uint64_t cap = a.stats ? static_cast<uint64_t>(num_cus()) * 8 : 0x7FFFFFFFull;
  if (blocks > cap) blocks = cap;
  const dim3 grid(static_cast<unsigned>(blocks ? blocks : 1));
  if (a.S <= 8) return launch_vote<uint8_t>(a, grid, st);
  return launch_vote<uint16_t>(a, grid, st);
}

}  // namespace qe
