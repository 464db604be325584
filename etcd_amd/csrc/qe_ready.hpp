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
// qe_ready is the three passes of the record-list layer (qe_list.hpp):
//   count   k_ready_count: one wave per 4096-group chunk.  Lane l of round j
//           takes the groups 2 (64 j + l) and + 1 of the chunk: one 16-B load
//           per u64 row and one 2-B load per byte row, each instruction a
//           contiguous run of the row; the predicate of both groups; their
//           flag bytes (one 2-B store) into scratch; the chunk's count.  A
//           ragged last chunk, or rows that are not 16-B / 2-B aligned, take a
//           lane per group.
//   scan    k_collect_scan (qe_collect.hpp, launched by qe_ready);
//   fill    k_ready_fill: the layer's walk, its counts the flag bytes; a tile
//           loads the rows of its listed groups only and writes one record
//           per group, in lane order.
// The fill reads the flag byte instead of recomputing the predicate: it costs
// 2 B per group against the 87 B the predicate reads, and at the densities a
// host sees (few groups have a Ready) the fill then touches almost nothing.
//
// qe_ready_note and qe_advance are elementwise: a thread per group and a
// thread per record.  The kernels that are no templates (k_ready_count,
// k_ready_note, k_advance) are defined in qe_inst_ready.hip.
#pragma once
#include "qe_list.hpp"

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
  RunCut<(E > 0 ? E : 1)> ec, ac;
  if constexpr (E > 0) {
    // a list holds 0xFFFFFFFF entries at most (qe_outbox rule 4): every ent_len
    // is a uint32, and run_cut takes a run's length from the low dwords.  The
    // cap in outbox_tile's wrap-safe form.  The apply list is cut first: with
    // the entries first k_ready_fill<4, 4> takes 129 VGPRs, a wave per SIMD less
    constexpr uint64_t lim = 0xFFFFFFFFull;
    const uint64_t chi = ahi - (off - 1) > lim ? off - 1 + lim : ahi;
    ac = run_cut<RM, E>(rf, rt, nr, li, off - 1, chi, apply);
    const uint64_t ehi = li - stable > lim ? stable + lim : li;
    ec = run_cut<RM, E>(rf, rt, nr, li, stable, ehi, ents);
    ent_count = ec.ents;
    ent_last = ec.last;
    apply_count = ac.ents;
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
  const auto [tbc, rem] = list_room(tb, a.cap, 64);
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
      bst32<kNT>(ec.len[k], mk_rsrc(a.o_ent_len + row, rem * 4), p4);
      bst64<kNT>(ec.term[k], mk_rsrc(a.o_ent_term + row, rem * 8), p8);
      bst32<kNT>(ac.len[k], mk_rsrc(a.o_apply_len + row, rem * 4), p4);
      bst64<kNT>(ac.term[k], mk_rsrc(a.o_apply_term + row, rem * 8), p8);
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

// The counts of the layer: the flag bytes k_ready_count left.
struct ReadyCounts {
  const uint8_t *flag;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const rsrc_t rf = mk_rsrc(flag + base, nc);
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) k[r] = bld8<kNT>(rf, list_elem(r)) != 0 ? 1u : 0u;
  }
};

template <int RM, int E>
__global__ __launch_bounds__(kBlock) void k_ready_fill(RDArgs a) {
  const int idx[RD_N] = {QE_STAT_GROUPS, QE_STAT_READY_ENTRIES, QE_STAT_READY_APPLY,
                         QE_STAT_READY_MUST_SYNC, QE_STAT_CHECKSUM};
  list_fill_walk<ready_tile<RM, E>>(a, idx, ReadyCounts{a.flag});
}

}  // namespace qe
