// qe_step.hpp — what the receiver-side step kernels share (k_tick, k_follow,
// k_vote, k_snap, k_compact; each in a header of its own on this one): the
// tile prologue, the header part of becomeFollower(m.Term, from) for a
// message from a leader, raftLog.term over a term-run table in registers, the
// cut of an entry range into the table's runs (qe_ready's lists), and the
// result / events rows every tile ends with.
//
// Two more pieces are the same text in two kernels and stay written out
// there: the term preamble (lower / higher / lead_same / proceed / bf, k_follow
// and k_snap) and the run-table load (k_follow and k_compact).  As functions,
// in any of the forms tried (a struct of five bools, reference arguments; one
// helper per row array), they change the register allocation of their callers:
// k_follow by one or two VGPRs, k_compact<16> from 153 VGPRs to 464 with 208
// AGPRs.  The callee's short-circuit and per-row control flow is simplified on
// its own before it is inlined, where the kernels' is simplified in place.
//
// The house idiom: one lane per group, one wave per 64-group tile (a capped
// grid walks, qe_launch.hpp tile_grid), per-tile buffer descriptors, a
// conditional access = an unconditional one whose offset is pushed out of
// range, rows read by need under ballots, a row stored only under the ballot
// of the lanes that changed it, every store after every load of the tile.
// Every row is touched once per launch: the accesses go non-temporal.  The
// statistics are wave sums (qe_device.hpp wave_stats_add): no LDS, no scratch.
#pragma once
#include "qe_tile.hpp"

namespace qe {

int hip_status(hipError_t e);

// Tile t of a walk: its first group, its group count (ragged at the end),
// the lane's 8-byte offset, whether the lane holds a group, and the group's
// global id.  `const auto [g0, n, o8, live, gid] = tile_at(...)`.
struct Tile {
  uint64_t g0;
  uint32_t n, o8;
  bool live;
  uint64_t gid;
};
__device__ __forceinline__ Tile tile_at(uint64_t G, uint64_t goff, uint64_t t, uint32_t lane) {
  const uint64_t g0 = t * 64;
  const uint32_t n = tile_n(G, t);
  return {g0, n, lane * 8, lane < n, goff + g0 + lane};
}
// The tile's message types: a lane has a message when its type is not 0
// (QE_LMSG_NONE, QE_VMSG_NONE, QE_SMSG_NONE).
__device__ __forceinline__ uint32_t msg_type(const uint8_t *type, uint64_t g0, uint32_t n,
                                             uint32_t lane) {
  return bld8<kNT>(mk_rsrc(type + g0, n), lane);
}

// The header rows of the groups a message went through (`ok`; `okbf` those
// that became followers, `w_term` those at a higher term): term and vote,
// state and transferee, lead, each under its ballot.
template <class A>
__device__ __forceinline__ void become_follower_stores(const A &a, uint64_t g0, uint32_t n,
                                                       uint32_t lane, bool w_term, bool okbf,
                                                       bool ok, uint64_t mterm, uint32_t st,
                                                       uint32_t from) {
  if (__builtin_amdgcn_ballot_w64(w_term)) {
    bst64<kNT>(mterm, mk_rsrc(a.term + g0, n * 8), w_term ? lane * 8 : kOOB);
    bst8<kNT>(0xFFu, opt_rsrc(a.vote, g0, n), w_term ? lane : kOOB);
  }
  if (__builtin_amdgcn_ballot_w64(okbf)) {
    const bool w_st = okbf && st != QE_STATE_FOLLOWER;
    bst8<kNT>(QE_STATE_FOLLOWER, mk_rsrc(a.state + g0, n), w_st ? lane : kOOB);
    bst8<kNT>(0xFFu, opt_rsrc(a.transferee, g0, n), okbf ? lane : kOOB);
  }
  if (__builtin_amdgcn_ballot_w64(ok))
    bst8<kNT>(from, mk_rsrc(a.lead + g0, n), ok ? lane : kOOB);
}

// raftLog.term (raft/log.go:265-285) over the runs in registers
// (oracle/quorum_oracle.c orc_log_term).
template <int RM>
__device__ __forceinline__ uint64_t run_term_at(const uint64_t (&rf)[RM], const uint64_t (&rt)[RM],
                                                uint32_t nr, uint64_t li, uint64_t i) {
  uint64_t t = 0;
#pragma unroll
  for (int r = 0; r < RM; r++) t = (static_cast<uint32_t>(r) < nr && i >= rf[r]) ? rt[r] : t;
  return (nr == 0 || i < rf[0] || i > li) ? 0 : t;
}

// The entries (i, hi] cut into the table's runs (the last run ends at li), at
// most E of them, for the lanes with `on`: qe_outbox rule 4.  -> len / term:
// the length and the term of each listed run, 0 past the last; the entries
// listed; the term of the last listed run.  (qe_ready's two lists; outbox_tile
// holds the same cut written out, see there.)
template <int E>
struct RunCut {
  uint32_t len[E];
  uint64_t term[E];
  uint64_t ents, last;
};
template <int RM, int E>
__device__ __forceinline__ RunCut<E> run_cut(const uint64_t (&rf)[RM], const uint64_t (&rt)[RM],
                                             uint32_t nr, uint64_t li, uint64_t i, uint64_t hi,
                                             bool on) {
  uint32_t j = 0;
  RunCut<E> c = {};
#pragma unroll
  for (int r = 0; r < RM; r++) {
    const uint64_t end = (r + 1 < RM && static_cast<uint32_t>(r + 1) < nr) ? rf[r + 1] - 1 : li;
    const uint64_t lo = rf[r] > i ? rf[r] : i + 1, e = end < hi ? end : hi;
    const bool ne = on && static_cast<uint32_t>(r) < nr && i < hi && lo <= e;
    const uint32_t len = static_cast<uint32_t>(e) - static_cast<uint32_t>(lo) + 1u;
    const bool in = ne && j < static_cast<uint32_t>(E);
#pragma unroll
    for (int k = 0; k < E; k++) {
      const bool sel = ne && j == static_cast<uint32_t>(k);
      c.len[k] = sel ? len : c.len[k];
      c.term[k] = sel ? rt[r] : c.term[k];
    }
    c.ents += in ? len : 0u;
    c.last = in ? rt[r] : c.last;
    j += ne ? 1u : 0u;
  }
  return c;
}

// What every tile ends with: the result of every group, and its QE_TEV_*
// events where the caller asked for them.
__device__ __forceinline__ void st_result_events(uint8_t *result, uint8_t *events, uint64_t g0,
                                                 uint32_t n, uint32_t lane, uint32_t res,
                                                 uint32_t ev) {
  bst8<kNT>(res, mk_rsrc(result + g0, n), lane);
  bst8<kNT>(ev, opt_rsrc(events, g0, n), lane);
}

}  // namespace qe
