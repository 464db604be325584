// qe_inst_tick.hip — per-slot-count instantiations of the tick kernel
// (qe_tick.hpp).  Compiled once per S (1..16) with -DQE_S=<S>, in objects of
// its own: the Progress kernels' objects (qe_inst_prog.hip) do not see it.
#include "qe_tick.hpp"

#ifndef QE_S
#error "compile with -DQE_S=<slots>"
#endif

namespace qe {

namespace {
constexpr int S = QE_S;
using MT = std::conditional<(S <= 8), uint8_t, uint16_t>::type;
}  // namespace

// One tile per wave (qe_launch.hpp tile_grid).
template <int N>
int dispatch_tick(const TArgs &a, bool masked, bool joint, hipStream_t st) {
  static_assert(N == S, "one slot count per object");
  const dim3 grid(tile_grid(a.G, num_cus(), a.stats != nullptr));
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_tick<S, MT, m(), j()>), grid, dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}
template int dispatch_tick<S>(const TArgs &, bool, bool, hipStream_t);

}  // namespace qe
