// qe_inst_prog.hip — per-slot-count instantiations of the Progress state
// machine kernels (qe_progress.hpp).  Compiled once per S (1..16) with
// -DQE_S=<S>, separately from qe_inst.hip so the two kernel families rebuild
// independently.
#include "qe_dispatch.hpp"

#ifndef QE_S
#error "compile with -DQE_S=<slots>"
#endif

namespace qe {

namespace {
constexpr int S = QE_S;
using MT = std::conditional<(S <= 8), uint8_t, uint16_t>::type;

// qe_progress_send and qe_check_quorum: the chunk plan of qe_launch.hpp with
// up to kSendTPW tiles per wave (a tiles_per_wave override is floored at 2 too)
ChunkPlan send_plan(uint64_t G) {
  return chunk_plan((G + 63) / 64, num_cus(), g_tiles_per_wave, kSendTPW, true);
}

// one tile per wave: the grid of the kernels that are not chunked
dim3 tile_grid(uint64_t G) { return dim3(grid_for((G + 63) / 64, 0, 1)); }
}  // namespace

template <int RM, bool ACCT, bool RD, int WPB = kBlock / 64, bool P = false, bool N16 = false>
static int launch_progress_step_p(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  // the same waves as the 4-wave grid, in blocks of WPB waves
  const uint64_t nb = static_cast<uint64_t>(grid_for((a.G + 63) / 64, 0, 1)) * ((kBlock / 64) / WPB);
  const dim3 grid(static_cast<unsigned>(nb < 0x7FFFFFFFull ? nb : 0x7FFFFFFFull));
  const dim3 blk(64 * WPB);
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_progress_step<S, MT, m(), j(), RM, ACCT, RD, WPB, P, N16>), grid, blk, 0, st, a);
    return hip_status(hipGetLastError());
  });
}

// ABI 8, the 16-bit Inflights form (host-checked: F <= 8, S <= 9, at most 4
// log runs): the pipelined kernels, and the rolled one for the byte count
static int launch_progress_step_n16(const PArgs &a, bool acct, bool masked, bool joint,
                                    hipStream_t st) {
  if constexpr (S <= QE_RING16_MAX_SLOTS) {
    if (acct) return launch_progress_step_p<4, true, true, kBlock / 64, false, true>(a, masked, joint, st);
    if (a.read_acks) return launch_progress_step_p<4, false, true, kBlock / 64, true, true>(a, masked, joint, st);
    return launch_progress_step_p<4, false, false, kBlock / 64, true, true>(a, masked, joint, st);
  }
  return QE_EINVAL;
}

// the pipelined slot loop (qe_progress.hpp) for rings in row form, up to 9
// slots and the 4-run table (3 waves/SIMD; with the 8-run table it needs
// 176-195 VGPRs from S = 6, 2 waves); the rolled loop otherwise
template <int RM, bool ACCT, bool RD, int WPB = kBlock / 64>
static int launch_progress_step(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  if constexpr (S <= 9 && RM <= 4 && !ACCT) {
    if (a.F <= kRingChunk) return launch_progress_step_p<RM, ACCT, RD, WPB, true>(a, masked, joint, st);
  }
  return launch_progress_step_p<RM, ACCT, RD, WPB, false>(a, masked, joint, st);
}

static int launch_progress_send(PArgs a, hipStream_t st) {
  const ChunkPlan plan = send_plan(a.G);
  if (plan.status) return plan.status;
  a.chunk = plan.chunk;
  if constexpr (S <= QE_RING16_MAX_SLOTS) {
    if (a.infl16) {
      hipLaunchKernelGGL((k_progress_send<S, MT, true>), dim3(plan.blocks), dim3(kBlock), 0, st, a);
      return hip_status(hipGetLastError());
    }
  }
  hipLaunchKernelGGL((k_progress_send<S, MT>), dim3(plan.blocks), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

static int launch_check_quorum(PArgs a, bool masked, bool joint, hipStream_t st) {
  const ChunkPlan plan = send_plan(a.G);
  if (plan.status) return plan.status;
  a.chunk = plan.chunk;
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_check_quorum<S, MT, m(), j()>), dim3(plan.blocks), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

template <bool RD>
static int step_runs(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  if (a.R <= 4) return launch_progress_step<4, false, RD>(a, masked, joint, st);
  if (a.R <= 8) return launch_progress_step<8, false, RD>(a, masked, joint, st);
  // the 16-run kernel: one wave per block
  return launch_progress_step<QE_MAX_LOG_RUNS, false, RD, 1>(a, masked, joint, st);
}

static int launch_read_index(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_read_index<S, MT, m(), j()>), tile_grid(a.G), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

template <bool ACCT, bool N16 = false>
static int launch_propose(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  if constexpr (!N16 && S <= QE_RING16_MAX_SLOTS) {
    if (a.infl16) return launch_propose<ACCT, true>(a, masked, joint, st);
  }
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_propose<S, MT, m(), j(), ACCT, N16>), tile_grid(a.G), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

template <bool ACCT, bool N16 = false>
static int launch_switch_config(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  if constexpr (!N16 && S <= QE_RING16_MAX_SLOTS) {
    if (a.infl16) return launch_switch_config<ACCT, true>(a, masked, joint, st);
  }
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_switch_config<S, MT, m(), j(), ACCT, N16>), tile_grid(a.G), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

static int launch_become_leader(const PArgs &a, bool masked, bool joint, hipStream_t st) {
  return with_quorum_form(masked, joint, [&](auto m, auto j) {
    hipLaunchKernelGGL((k_become_leader<S, MT, m(), j()>), tile_grid(a.G), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

static int launch_heartbeat(const PArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((k_heartbeat<S, MT>), tile_grid(a.G), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int N>
int dispatch_progress(const PArgs &a, ProgressOp op, bool acct, bool masked, bool joint,
                      hipStream_t st) {
  static_assert(N == S, "one slot count per object");
  switch (op) {
    case ProgressOp::Send: return launch_progress_send(a, st);
    case ProgressOp::CheckQuorum: return launch_check_quorum(a, masked, joint, st);
    case ProgressOp::ReadIndex: return launch_read_index(a, masked, joint, st);
    case ProgressOp::Propose:
      if (!acct) return launch_propose<false>(a, masked, joint, st);
      return launch_propose<true>(a, masked, joint, st);
    case ProgressOp::Heartbeat: return launch_heartbeat(a, st);
    case ProgressOp::SwitchConfig:
      if (!acct) return launch_switch_config<false>(a, masked, joint, st);
      return launch_switch_config<true>(a, masked, joint, st);
    case ProgressOp::BecomeLeader: return launch_become_leader(a, masked, joint, st);
    case ProgressOp::Step: break;
  }
  // run table (staged in LDS, l_run): 4 runs cover the common leader log (one
  // or two older terms before the current one); 8 keep the block's LDS at
  // 52 KB (3 blocks per CU at S = 5, where 16 runs' 84 KB allow one);
  // up to QE_MAX_LOG_RUNS otherwise
  // ReadIndex tracking (a.read_acks) takes a variant of its own: its queue
  // state costs registers the rounds without reads should not pay
  if (a.infl16) return launch_progress_step_n16(a, acct, masked, joint, st);
  if (acct) return launch_progress_step<QE_MAX_LOG_RUNS, true, true>(a, masked, joint, st);
  if (a.read_acks) return step_runs<true>(a, masked, joint, st);
  return step_runs<false>(a, masked, joint, st);
}
template int dispatch_progress<S>(const PArgs &, ProgressOp, bool, bool, bool, hipStream_t);

}  // namespace qe
