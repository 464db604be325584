// qe_inst_readstates.hip — the ReadState kernels (qe_readstates.hpp):
// k_read_note, k_read_states_count and k_read_states_fill.  None depends on
// the slot count at compile time, so this object is compiled once, not per
// QE_S.
#include "qe_readstates.hpp"

namespace qe {

// qe_read_note: readOnly.addRequest's bookkeeping (raft/read_only.go:56-63),
// a thread per group.
__global__ __launch_bounds__(kBlock) void k_read_note(RNoteArgs a) {
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g < a.G;
       g += static_cast<uint64_t>(gridDim.x) * kBlock) {
    if (a.result[g] != QE_RI_QUEUED) continue;
    const uint64_t e = g * a.cap + a.ctx[g] % a.cap;
    a.req_index[e] = a.index[g];
    a.req_from[e] = a.from ? a.from[g] : 0xFFu;
  }
}

__global__ __launch_bounds__(kBlock) void k_read_states_count(RSArgs a) {
  list_count_block(a.G, a.counts, ReadStatesCounts{a});
}

__global__ __launch_bounds__(kBlock) void k_read_states_fill(RSArgs a) {
  const int idx[RS_N] = {QE_STAT_GROUPS, QE_STAT_READ_STATE, QE_STAT_READ_RESP,
                         QE_STAT_READ_TERM_COMMIT, QE_STAT_CHECKSUM};
  list_fill_walk<read_states_tile>(a, idx, ReadStatesCounts{a});
}

int dispatch_read_note(const RNoteArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_read_note, dim3(elem_grid(a.G, num_cus())), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// One block per chunk; qe_read_states has checked that the chunks fit a launch.
int dispatch_read_states_count(const RSArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_read_states_count, dim3(static_cast<unsigned>(a.nb)), dim3(kBlock), 0, st,
                     a);
  return hip_status(hipGetLastError());
}

int dispatch_read_states_fill(const RSArgs &a, hipStream_t st) {
  const dim3 grid(list_fill_grid(a.nb, num_cus(), a.stats != nullptr));
  hipLaunchKernelGGL(k_read_states_fill, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
