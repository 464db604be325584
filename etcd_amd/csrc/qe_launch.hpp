// qe_launch.hpp — the launch rules every kernel family shares: the
// tiles-per-wave chunk plan, the one-tile-per-wave grid with its statistics
// cap, and the helpers that turn run-time choices (slot count, quorum form,
// non-temporal bits) into compile-time constants.  Plain C++17 with no HIP in
// it, so a host-only program can include it (tests/cpp/chunk_plan_test.cpp).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/etcd_quorum.h"

namespace qe {

constexpr int kBlock = 256;

// A chunked kernel gives each wave `chunk` consecutive 64-group tiles and
// keeps the next tile's loads in flight while one is decided.  The automatic
// chunk gives every CU 32 waves when the batch allows it and is at least 2,
// so the two register sets still overlap; it never exceeds the kernel's
// `max_tpw`.  A qe_tune("tiles_per_wave", T > 0) override replaces the
// automatic chunk.  The stream kernels take it as given (T = 1 is a chunk of
// 1); send, check_quorum and confchange floor it at 2 as well
// (`floor_override`).
struct ChunkPlan {
  int status;  // QE_OK, or QE_ERANGE when the grid would pass 2^31 - 1 blocks
  uint32_t chunk, blocks;
};

inline ChunkPlan chunk_plan(uint64_t tiles, int cus, int tpw_override, uint32_t max_tpw,
                            bool floor_override) {
  uint64_t chunk;
  if (tpw_override > 0) {
    chunk = static_cast<uint64_t>(tpw_override);
    if (floor_override && chunk < 2) chunk = 2;
  } else {
    const uint64_t waves = static_cast<uint64_t>(cus) * 32;
    chunk = (tiles + waves - 1) / waves;
    if (chunk < 2) chunk = 2;
  }
  if (chunk > max_tpw) chunk = max_tpw;
  const uint64_t per_block = (kBlock / 64) * chunk;
  const uint64_t blocks = (tiles + per_block - 1) / per_block;
  if (blocks > 0x7FFFFFFFull) return {QE_ERANGE, 0, 0};
  return {QE_OK, static_cast<uint32_t>(chunk), static_cast<uint32_t>(blocks)};
}

// The grid of a kernel that gives each wave one 64-group tile (qe_tick and
// the step kernels): a block per kBlock / 64 tiles, at least one.  With
// statistics it is capped at 8 blocks per CU and the waves walk, since every
// wave ends with one atomic per counter; without, at the 2^31 - 1 blocks of a
// launch.
inline uint32_t tile_grid(uint64_t groups, int cus, bool stats) {
  const uint64_t tiles = (groups + 63) / 64;
  uint64_t blocks = (tiles + (kBlock / 64) - 1) / (kBlock / 64);
  const uint64_t cap = stats ? static_cast<uint64_t>(cus) * 8 : 0x7FFFFFFFull;
  if (blocks > cap) blocks = cap;
  return static_cast<uint32_t>(blocks ? blocks : 1);
}

// The grid of a record list's fill pass (qe_list.hpp): one block per chunk;
// with statistics it is capped at 8 blocks per CU and the blocks walk, since
// every wave ends with one atomic per counter.  The caller has checked that
// the chunks fit a launch.
inline uint32_t list_fill_grid(uint64_t chunks, int cus, bool stats) {
  const uint64_t cap = stats ? static_cast<uint64_t>(cus) * 8 : chunks;
  return static_cast<uint32_t>(chunks < cap ? chunks : cap);
}

// The grid of an element-wise kernel: a thread per element, at least one
// block and at most 8 per CU (the blocks walk).
inline uint32_t elem_grid(uint64_t n, int cus) {
  const uint64_t cap = static_cast<uint64_t>(cus) * 8;
  const uint64_t need = (n + kBlock - 1) / kBlock;
  return static_cast<uint32_t>(need < cap ? (need ? need : 1) : cap);
}

// The three quorum forms the kernels are built for: f(MASKED, JOINT) with
// std::bool_constant arguments — a plain majority of every slot, a majority
// of inc_mask, or the joint quorum of inc_mask and out_mask.
template <class F>
inline int with_quorum_form(bool masked, bool joint, F &&f) {
  if (joint) return f(std::true_type{}, std::true_type{});
  if (masked) return f(std::true_type{}, std::false_type{});
  return f(std::false_type{}, std::false_type{});
}

// qe_tune("nontemporal"): f(NTL, NTS), bit 0 the loads, bit 1 the stores.
template <class F>
inline int with_nontemporal(int bits, F &&f) {
  switch (bits & 3) {
    case 1: return f(std::true_type{}, std::false_type{});
    case 2: return f(std::false_type{}, std::true_type{});
    case 3: return f(std::true_type{}, std::true_type{});
    default: return f(std::false_type{}, std::false_type{});
  }
}

// Dispatch by slot count: f(std::integral_constant<int, S>) for S in
// 1..QE_MAX_SLOTS, QE_EINVAL otherwise.
template <int N>
using slots_c = std::integral_constant<int, N>;

template <class F>
inline int with_slots(uint32_t S, F &&f) {
  static_assert(QE_MAX_SLOTS == 16, "one case per slot count");
  switch (S) {
    case 1: return f(slots_c<1>{});
    case 2: return f(slots_c<2>{});
    case 3: return f(slots_c<3>{});
    case 4: return f(slots_c<4>{});
    case 5: return f(slots_c<5>{});
    case 6: return f(slots_c<6>{});
    case 7: return f(slots_c<7>{});
    case 8: return f(slots_c<8>{});
    case 9: return f(slots_c<9>{});
    case 10: return f(slots_c<10>{});
    case 11: return f(slots_c<11>{});
    case 12: return f(slots_c<12>{});
    case 13: return f(slots_c<13>{});
    case 14: return f(slots_c<14>{});
    case 15: return f(slots_c<15>{});
    case 16: return f(slots_c<16>{});
    default: return QE_EINVAL;
  }
}

template <int N>
using runs_c = std::integral_constant<int, N>;

// Dispatch by the run-capacity bucket of a kernel that holds the run table in
// registers: f(runs_c<RM>) for the first RM of 4, 8, 16 that log_runs fits.
template <class F>
inline int with_run_bucket(uint32_t log_runs, F &&f) {
  static_assert(QE_MAX_LOG_RUNS == 16, "the last bucket holds every run table");
  if (log_runs <= 4) return f(runs_c<4>{});
  if (log_runs <= 8) return f(runs_c<8>{});
  return f(runs_c<16>{});
}

// Dispatch by the run capacity of a record (msg_runs, ent_runs): f(runs_c<E>)
// for E in 0..QE_MAX_MSG_RUNS; the caller has refused a larger one.
template <class F>
inline int with_msg_runs(uint32_t runs, F &&f) {
  static_assert(QE_MAX_MSG_RUNS == 4, "one case per run capacity");
  switch (runs) {
    case 0: return f(runs_c<0>{});
    case 1: return f(runs_c<1>{});
    case 2: return f(runs_c<2>{});
    case 3: return f(runs_c<3>{});
    default: return f(runs_c<4>{});
  }
}

}  // namespace qe
