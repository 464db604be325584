// qe_ready.hpp — qe_ready_note, qe_ready and qe_advance: the storage half of
// RawNode.Ready() / Advance() on resident rows (include/etcd_quorum.h states
// the rules).
//
// HasReady and readyWithoutAccept (raft/rawnode.go:133-170, raft/node.go:
// 562-593) compare the group's HardState and SoftState with the ones the last
// Advance kept, and list the unstable entries, the committed entries not yet
// applied and a pending snapshot.  Everything that takes is resident: term,
// vote, lead, state, the log rows, and the eight rows of qe_ready_state.
//
// qe_ready is qe_outbox's three passes on qe_outbox's machinery:
//   count   k_ready_count: one wave per 4096-group chunk.  Lane l of round j
//           takes the groups 2 (64 j + l) and + 1 of the chunk: one 16-B load
//           per u64 row and one 2-B load per byte row, each instruction a
//           contiguous run of the row; the predicate of both groups; their
//           flag bytes (one 2-B store) into scratch; the chunk's count.  A
//           ragged last chunk, or rows that are not 16-B / 2-B aligned, take a
//           lane per group.
//   scan    k_collect_scan (qe_collect.hpp, launched by qe_ready);
//   fill    k_ready_fill: k_outbox_fill's walk over the flag bytes
//           (chunk_tile_counts reads them as a one-slot mask); a tile loads the
//           rows of its listed groups only and writes one record per group, in
//           lane order: a wave's stores are one contiguous run.  No block
//           waits for another.
// The fill reads the flag byte instead of recomputing the predicate: it costs
// 2 B per group against the 87 B the predicate reads, and at the densities a
// host sees (few groups have a Ready) the fill then touches almost nothing.
//
// qe_ready_note and qe_advance are elementwise: a thread per group and a
// thread per record.  The kernels that are no templates (k_ready_count,
// k_ready_note, k_advance) are defined in qe_inst_ready.hip.
#pragma once
#include "qe_outbox.hpp"

namespace qe {

constexpr uint64_t kReadySalt = 0x8CB92BA72F3D8DD7ull;

struct RDArgs {
  uint64_t G, goff, stride;
  uint32_t R, S;
  uint32_t max_apply;
  uint32_t vec;  // every row allows the pair loads of the count pass
  uint64_t nb;   // chunks
  // qe_progress
  const uint64_t *committed, *last_index, *run_first, *run_term;
  const uint8_t *run_count;
  // qe_follower
  const uint64_t *term;
  const uint8_t *state, *lead, *vote;
  // qe_ready_state
  const uint64_t *stable, *applied, *snap_pending, *prev_term, *prev_commit;
  const uint8_t *prev_vote, *prev_lead, *prev_state;
  const uint8_t *pending;
  // qe_ready_out
  uint64_t cap;
  uint64_t *o_group, *o_term, *o_commit;
  uint8_t *o_vote, *o_lead, *o_state, *o_flags;
  uint64_t *o_ent_first, *o_ent_count, *o_ent_last_term, *o_apply_first, *o_apply_count,
      *o_snap_index;
  uint32_t *o_ent_len, *o_apply_len;
  uint64_t *o_ent_term, *o_apply_term;
  // scratch
  const uint64_t *offsets;
  uint32_t *counts;
  uint8_t *flag;  // [G] 1 = listed
  uint64_t *stats;
};

struct RNArgs {
  uint64_t G;
  const uint8_t *follow_result, *snap_result;
  const uint64_t *append_from, *resp_index;
  uint64_t *stable, *snap_pending;
};

struct ADArgs {
  uint64_t G, goff, stride, cap;
  uint32_t R, S;
  const uint64_t *count;
  // the list
  const uint64_t *group, *term, *commit;
  const uint8_t *vote, *lead, *state, *flags;
  const uint64_t *ent_first, *ent_count, *ent_last_term, *apply_first, *apply_count, *snap_index;
  // qe_progress
  const uint64_t *committed, *last_index, *run_first, *run_term;
  const uint8_t *run_count;
  // qe_ready_state
  uint64_t *stable, *applied, *snap_pending, *prev_term, *prev_commit;
  uint8_t *prev_vote, *prev_lead, *prev_state;
  // AutoLeave
  const uint8_t *auto_leave, *cur_state;
  const uint64_t *pending_conf_index;
  uint8_t *result;
};

// defined in qe_inst_ready.hip
int dispatch_ready_note(const RNArgs &a, hipStream_t st);
int dispatch_ready_count(const RDArgs &a, hipStream_t st);
int dispatch_ready_fill(const RDArgs &a, uint32_t ent_runs, hipStream_t st);
int dispatch_advance(const ADArgs &a, hipStream_t st);

// A slot row's value with every value that is no slot taken as None.
__device__ __forceinline__ uint32_t rd_slot(uint32_t v, uint32_t S) { return v < S ? v : 0xFFu; }

// What one group's Ready holds besides its entries: QE_RD_SOFT / _HARD /
// _MUST_SYNC / _SNAP, and in bit 8 whether the group is listed at all.
constexpr uint32_t kRdListed = 0x100u;
__device__ __forceinline__ uint32_t rd_flags(uint32_t S, uint64_t term, uint32_t vote,
                                             uint64_t commit, uint32_t lead, uint32_t state,
                                             uint64_t stable, uint64_t li, uint64_t applied,
                                             uint64_t rf0, uint64_t snapp, uint64_t pterm,
                                             uint64_t pcommit, uint32_t pvote, uint32_t plead,
                                             uint32_t pstate, uint32_t pending) {
  const uint32_t v = rd_slot(vote, S), pv = rd_slot(pvote, S);
  const bool hard_changed = term != pterm || v != pv || commit != pcommit;
  const bool hard_empty = term == 0 && v == 0xFFu && commit == 0;
  const bool soft = rd_slot(lead, S) != rd_slot(plead, S) || state != pstate;
  const bool hard = !hard_empty && hard_changed;
  const bool ents = li > stable;
  const uint64_t a1 = applied + 1, f1 = rf0 + 1, off = a1 > f1 ? a1 : f1;
  const bool apply = commit + 1 > off;
  const bool sync = ents || v != pv || term != pterm;
  const bool listed = soft || hard || snapp != 0 || ents || apply || pending != 0;
  return (soft ? QE_RD_SOFT : 0u) | (hard ? QE_RD_HARD : 0u) | (sync ? QE_RD_MUST_SYNC : 0u) |
         (snapp != 0 ? QE_RD_SNAP : 0u) | (listed ? kRdListed : 0u);
}

enum { RD_RECORDS, RD_ENTRIES, RD_APPLY, RD_SYNC, RD_CSUM, RD_N };

// (i, hi] cut into the table's runs (the last run ends at li), at most E of
// them: qe_outbox rule 4.  -> the entries listed; `last` the term of the last
// listed run.
template <int RM, int E>
__device__ __forceinline__ uint64_t rd_cut(const uint64_t (&rf)[RM], const uint64_t (&rt)[RM],
                                           uint32_t nr, uint64_t li, uint64_t i, uint64_t hi,
                                           bool on, uint32_t (&el)[E], uint64_t (&et)[E],
                                           uint64_t &last) {
  uint32_t j = 0;
  uint64_t ents = 0;
#pragma unroll
  for (int k = 0; k < E; k++) {
    el[k] = 0;
    et[k] = 0;
  }
  last = 0;
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
      el[k] = sel ? len : el[k];
      et[k] = sel ? rt[r] : et[k];
    }
    ents += in ? len : 0u;
    last = in ? rt[r] : last;
    j += ne ? 1u : 0u;
  }
  return ents;
}

// Tile t, whose first record has position tb.
template <int RM, int E>
__device__ __forceinline__ void ready_tile(const RDArgs &a, uint64_t t, uint64_t tb, uint32_t lane,
                                           uint64_t (&cnt)[RD_N]) {
  const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
  // ---- 1. who is listed ----
  const bool has = live && bld8<kNT>(mk_rsrc(a.flag + g0, n), lane) != 0;
  const uint32_t h1 = has ? lane : kOOB, h8 = has ? o8 : kOOB;
  // ---- 2. the rows of the listed groups ----
  const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), h8);
  const uint64_t commit = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), h8);
  const uint64_t li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), h8);
  const uint64_t stable = bld64<kNT>(mk_rsrc(a.stable + g0, n * 8), h8);
  const uint64_t applied = bld64<kNT>(mk_rsrc(a.applied + g0, n * 8), h8);
  const uint64_t snapp = bld64<kNT>(mk_rsrc(a.snap_pending + g0, n * 8), h8);
  const uint64_t pterm = bld64<kNT>(mk_rsrc(a.prev_term + g0, n * 8), h8);
  const uint64_t pcommit = bld64<kNT>(mk_rsrc(a.prev_commit + g0, n * 8), h8);
  const uint32_t vote = a.vote ? bld8<kNT>(mk_rsrc(a.vote + g0, n), h1) : 0xFFu;
  const uint32_t lead = bld8<kNT>(mk_rsrc(a.lead + g0, n), h1);
  const uint32_t state = bld8<kNT>(mk_rsrc(a.state + g0, n), h1);
  const uint32_t pvote = bld8<kNT>(mk_rsrc(a.prev_vote + g0, n), h1);
  const uint32_t plead = bld8<kNT>(mk_rsrc(a.prev_lead + g0, n), h1);
  const uint32_t pstate = bld8<kNT>(mk_rsrc(a.prev_state + g0, n), h1);
  uint32_t nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), h1);
  nr = nr < a.R ? nr : a.R;
  uint64_t rf[RM], rt[RM];
#pragma unroll
  for (int r = 0; r < RM; r++) {
    rf[r] = 0;
    rt[r] = 0;
    if (static_cast<uint32_t>(r) < a.R) {
      const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
      rf[r] = bld64<kNT>(mk_rsrc(a.run_first + row, n * 8), h8);
      rt[r] = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), h8);
    }
  }
  // ---- 3. the record ----
  const uint32_t f = rd_flags(a.S, term, vote, commit, lead, state, stable, li, applied, rf[0],
                              snapp, pterm, pcommit, pvote, plead, pstate, 0u);
  // Entries: (stable, last_index]
  const bool ents = has && li > stable;
  // CommittedEntries: [off, committed], max_apply of them at most
  const uint64_t a1 = applied + 1, f1 = rf[0] + 1, off = a1 > f1 ? a1 : f1;
  const bool apply = has && commit + 1 > off;
  const uint64_t want = commit + 1 - off;
  const uint64_t ahi = (a.max_apply && want > a.max_apply) ? off + a.max_apply - 1 : commit;
  uint64_t ent_count, ent_last, apply_count;
  uint32_t el[E > 0 ? E : 1], al[E > 0 ? E : 1];
  uint64_t et[E > 0 ? E : 1], at[E > 0 ? E : 1];
  if constexpr (E > 0) {
    uint64_t alast;
    ent_count = rd_cut<RM, E>(rf, rt, nr, li, stable, li, ents, el, et, ent_last);
    apply_count = rd_cut<RM, E>(rf, rt, nr, li, off - 1, ahi, apply, al, at, alast);
  } else {
    ent_count = ents ? li - stable : 0;
    ent_last = ents ? run_term_at<RM>(rf, rt, nr, li, li) : 0;
    apply_count = apply ? ahi + 1 - off : 0;
  }
  const uint32_t flags = (f & 0xFFu) | ((ents && stable + ent_count < li) ? QE_RD_ENTS_CUT : 0u) |
                         ((apply && off + apply_count - 1 < commit) ? QE_RD_APPLY_CUT : 0u);
  const uint64_t apply_first = apply_count ? off : 0;
  const uint32_t v = rd_slot(vote, a.S), l = rd_slot(lead, a.S);
  // ---- 4. the stores: the records of the tile in lane order ----
  const uint64_t bal = __builtin_amdgcn_ballot_w64(has);
  const uint32_t pos = lane_rank(bal);
  const uint64_t tbc = tb < a.cap ? tb : a.cap;
  const uint32_t rem = static_cast<uint32_t>(a.cap - tbc < 64 ? a.cap - tbc : 64);
  const uint32_t p1 = has ? pos : kOOB, p4 = has ? pos * 4 : kOOB, p8 = has ? pos * 8 : kOOB;
  bst64<kNT>(gid, mk_rsrc(a.o_group + tbc, rem * 8), p8);
  bst64<kNT>(term, mk_rsrc(a.o_term + tbc, rem * 8), p8);
  bst64<kNT>(commit, mk_rsrc(a.o_commit + tbc, rem * 8), p8);
  bst8<kNT>(v, mk_rsrc(a.o_vote + tbc, rem), p1);
  bst8<kNT>(l, mk_rsrc(a.o_lead + tbc, rem), p1);
  bst8<kNT>(state, mk_rsrc(a.o_state + tbc, rem), p1);
  bst8<kNT>(flags, mk_rsrc(a.o_flags + tbc, rem), p1);
  bst64<kNT>(stable + 1, mk_rsrc(a.o_ent_first + tbc, rem * 8), p8);
  bst64<kNT>(ent_count, mk_rsrc(a.o_ent_count + tbc, rem * 8), p8);
  bst64<kNT>(ent_last, mk_rsrc(a.o_ent_last_term + tbc, rem * 8), p8);
  bst64<kNT>(apply_first, mk_rsrc(a.o_apply_first + tbc, rem * 8), p8);
  bst64<kNT>(apply_count, mk_rsrc(a.o_apply_count + tbc, rem * 8), p8);
  bst64<kNT>(snapp, mk_rsrc(a.o_snap_index + tbc, rem * 8), p8);
  if constexpr (E > 0) {
#pragma unroll
    for (int k = 0; k < E; k++) {
      const uint64_t row = static_cast<uint64_t>(k) * a.cap + tbc;
      bst32<kNT>(el[k], mk_rsrc(a.o_ent_len + row, rem * 4), p4);
      bst64<kNT>(et[k], mk_rsrc(a.o_ent_term + row, rem * 8), p8);
      bst32<kNT>(al[k], mk_rsrc(a.o_apply_len + row, rem * 4), p4);
      bst64<kNT>(at[k], mk_rsrc(a.o_apply_term + row, rem * 8), p8);
    }
  }
  if (a.stats) {
    uint64_t h = mix64((gid * kPhi) ^ kReadySalt ^ (static_cast<uint64_t>(flags) << 56) ^
                       (static_cast<uint64_t>(v) << 48) ^ (static_cast<uint64_t>(l) << 40) ^
                       (static_cast<uint64_t>(state) << 32));
    h = mix64(h ^ term);
    h = mix64(h ^ commit);
    h = mix64(h ^ (stable + 1));
    h = mix64(h ^ ent_count);
    h = mix64(h ^ ent_last);
    h = mix64(h ^ apply_first);
    h = mix64(h ^ apply_count);
    h = mix64(h ^ snapp);
    cnt[RD_RECORDS] += has ? 1u : 0u;
    cnt[RD_ENTRIES] += has ? ent_count : 0u;
    cnt[RD_APPLY] += has ? apply_count : 0u;
    cnt[RD_SYNC] += (has && (flags & QE_RD_MUST_SYNC)) ? 1u : 0u;
    cnt[RD_CSUM] += has ? h : 0u;
  }
}

// k_outbox_fill's walk with the flag bytes as the masks of one slot.
template <int RM, int E>
__global__ __launch_bounds__(kBlock) void k_ready_fill(RDArgs a) {
  __shared__ uint32_t tcnt[kObTiles];
  uint64_t cnt[RD_N] = {0, 0, 0, 0, 0};
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  OBArgs m{};
  m.G = a.G;
  m.S = 1;
  m.sent = a.flag;
  for (uint64_t c = blockIdx.x; c < a.nb; c += gridDim.x) {
    chunk_tile_counts(m, false, c, tcnt);
    __syncthreads();
    const uint32_t x = tcnt[lane];
    __syncthreads();  // (the next chunk's counts overwrite tcnt)
    uint32_t inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d, 64);
      if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    const uint32_t pre = inc - x;
    const uint64_t cbase = a.offsets[c];
    for (uint32_t k = 0; k < kObRounds; k++) {
      const uint32_t T = k * (kBlock / 64) + w;
      if (__builtin_amdgcn_readfirstlane(__shfl(x, T, 64)) == 0) continue;  // no record
      const uint64_t tb = cbase + __builtin_amdgcn_readfirstlane(__shfl(pre, T, 64));
      ready_tile<RM, E>(a, c * kObTiles + T, tb, lane, cnt);
    }
  }
  if (a.stats) {
    const int idx[RD_N] = {QE_STAT_GROUPS, QE_STAT_READY_ENTRIES, QE_STAT_READY_APPLY,
                           QE_STAT_READY_MUST_SYNC, QE_STAT_CHECKSUM};
    wave_stats_add<RD_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
