// qe_inst.hip — per-slot-count instantiations of the hot kernels.  Compiled
// once per S (1..16) with -DQE_S=<S> so the 16 variants build in parallel.
#include "qe_dispatch.hpp"

#ifndef QE_S
#error "compile with -DQE_S=<slots>"
#endif
#ifndef QE_PAIRS
#define QE_PAIRS ((QE_S) <= 8 ? 2 : 1)  // adjacent-group pairs per lane per tile
#endif

namespace qe {

namespace {
constexpr int S = QE_S;
using MT = std::conditional<(S <= 8), uint8_t, uint16_t>::type;

template <int MODE, bool VEC, bool NTL, bool NTS>
int launch_cv_k(const CVArgs &a, hipStream_t st) {
  constexpr int kPairs = QE_PAIRS;
  auto kern = k_commit_vote<S, MODE, MT, kPairs, VEC, NTL, NTS>;
  static int occ = occupancy(kern);
  const uint64_t npairs = (a.G + 1) / 2;
  const uint64_t tiles = (npairs + 64 * kPairs - 1) / (64 * kPairs);
  hipLaunchKernelGGL(kern, dim3(grid_for(tiles, occ, MODE == 2 ? 8 : 1)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// The stream kernels' chunk plan (qe_launch.hpp): up to QE_STREAM_TPW tiles per
// wave; a qe_tune("tiles_per_wave") override is taken as given, 1 included.
ChunkPlan stream_plan(uint64_t G) {
  return chunk_plan((G + 63) / 64, num_cus(), g_tiles_per_wave, QE_STREAM_TPW, false);
}

template <int MODE, bool NTL, bool NTS>
int launch_cv_stream(CVArgs a, hipStream_t st) {
  auto kern = k_cv_stream<S, MODE, MT, NTL, NTS>;
  const ChunkPlan plan = stream_plan(a.G);
  if (plan.status) return plan.status;
  a.chunk = plan.chunk;
  hipLaunchKernelGGL(kern, dim3(plan.blocks), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int MODE>
int launch_cv(const CVArgs &a, bool vec, hipStream_t st) {
  // default: the stream kernel (measured faster in every mode);
  // it addresses each 64-group tile through buffer descriptors and needs
  // no row alignment
  const int which = g_cv_kernel >= 0 ? g_cv_kernel : 1;
  if (which == 1)
    return with_nontemporal(g_nontemporal, [&](auto ntl, auto nts) {
      return launch_cv_stream<MODE, ntl(), nts()>(a, st);
    });
  if (!vec) return launch_cv_k<MODE, false, false, false>(a, st);
  return with_nontemporal(g_nontemporal, [&](auto ntl, auto nts) {
    return launch_cv_k<MODE, true, ntl(), nts()>(a, st);
  });
}
}  // namespace

// Every dispatch_<family><N> below is defined for this object's slot count
// alone and instantiated for it at the end of its family.
template <int N>
int dispatch_cv(const CVArgs &a, int mode, bool vec, hipStream_t st) {
  static_assert(N == S, "one slot count per object");
  switch (mode) {
    case 0: return launch_cv<0>(a, vec, st);
    case 1: return launch_cv<1>(a, vec, st);
    default: return launch_cv<2>(a, vec, st);
  }
}
template int dispatch_cv<S>(const CVArgs &, int, bool, hipStream_t);

template <bool J, bool M, bool V, bool NT>
static int launch_repl_k(const RArgs &a, hipStream_t st) {
  auto kern = k_replication<S, J, M, MT, V, NT>;
  static int occ = occupancy(kern);
  const uint64_t tiles = ((a.G + 1) / 2 + 63) / 64;
  hipLaunchKernelGGL(kern, dim3(grid_for(tiles, occ, 1)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// non-temporal state traffic whenever qe_tune("nontemporal") has both bits
template <bool J, bool M, bool V>
static int launch_repl(const RArgs &a, hipStream_t st) {
  if (V && (g_nontemporal & 3) == 3) return launch_repl_k<J, M, V, true>(a, st);
  return launch_repl_k<J, M, V, false>(a, st);
}

// Stream replication kernel (qe_repl.hpp); chunking as launch_cv_stream.
template <bool M, bool J, bool NTL, bool NTS>
static int launch_repl_stream(RArgs a, hipStream_t st) {
  auto kern = k_repl_stream<S, M, J, MT, NTL, NTS>;
  const ChunkPlan plan = stream_plan(a.G);
  if (plan.status) return plan.status;
  a.chunk = plan.chunk;
  hipLaunchKernelGGL(kern, dim3(plan.blocks), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int N>
int dispatch_repl(const RArgs &a, bool masked, bool joint, bool vec, hipStream_t st) {
  static_assert(N == S, "one slot count per object");
  if (g_repl_kernel != 0)  // default: stream kernel (no alignment requirement)
    return with_quorum_form(masked, joint, [&](auto m, auto j) {
      return with_nontemporal(g_nontemporal, [&](auto ntl, auto nts) {
        return launch_repl_stream<m(), j(), ntl(), nts()>(a, st);
      });
    });
  if (vec)
    return with_quorum_form(masked, joint,
                            [&](auto m, auto j) { return launch_repl<j(), m(), true>(a, st); });
  return with_quorum_form(masked, joint,
                          [&](auto m, auto j) { return launch_repl<j(), m(), false>(a, st); });
}
template int dispatch_repl<S>(const RArgs &, bool, bool, bool, hipStream_t);

template <int OPT>
static int launch_elec(const EArgs &a, hipStream_t st) {
  auto kern = k_election<S, MT, OPT>;
  static int occ = occupancy(kern);
  const uint64_t waves = (a.G + 63) / 64;
  hipLaunchKernelGGL(kern, dim3(grid_for(waves, occ, 1)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int N>
int dispatch_elec(const EArgs &a, hipStream_t st) {
  static_assert(N == S, "one slot count per object");
  const int opt = (a.flags & 3u) | (a.sresp ? 4 : 0) | (a.out ? 8 : 0);
  switch (opt) {
#define QE_E(o) \
  case o: return launch_elec<o>(a, st);
    QE_E(0) QE_E(1) QE_E(2) QE_E(3) QE_E(4) QE_E(5) QE_E(6) QE_E(7)
    QE_E(8) QE_E(9) QE_E(10) QE_E(11) QE_E(12) QE_E(13) QE_E(14)
#undef QE_E
    default: return launch_elec<15>(a, st);
  }
}
template int dispatch_elec<S>(const EArgs &, hipStream_t);

}  // namespace qe
