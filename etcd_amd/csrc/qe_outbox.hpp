// qe_outbox.hpp — qe_outbox: the messages one leader-side call sent, as a
// dense, ordered list of records (include/etcd_quorum.h states the rules).
//
// The step kernels report a send as mask bits; maybeSendAppend
// (raft/raft.go:432-492) and bcastHeartbeatWithCtx (:525-532) say what the
// message of a bit carries.  Everything a record needs is resident: the masks,
// msg_index or Next, the term-run log, committed, the sender's term.
//
// The three passes of the record-list layer (qe_list.hpp): k_outbox_count
// counts a chunk's records from the masks alone, k_outbox_fill recounts its
// chunk's tiles from the mask bytes and fills them.
// A tile: one lane per group; the masks, then term, the log's header and run
// table, snap_index and hb_ctx once per tile under the ballot of the lanes that
// need them; then the per-slot rows (index, or peer and next_before / next;
// hb_commit) of every slot in the tile's mask union; then, slot by slot, the
// records (the slot's base is the popcount of the earlier slots' ballots).
//
// RM is the run-capacity bucket (log_runs <= 4 / 8 / 16, as k_compact), E the
// message's run capacity (qe_outbox_out.msg_runs).  The slot count and the mask
// width are run-time values: one object, not one per QE_S.
#pragma once
#include "qe_list.hpp"

namespace qe {

constexpr uint32_t kObTileMax = 64 * QE_MAX_SLOTS;    // records of one tile at most
constexpr uint64_t kOutboxSalt = 0xC2B2AE3D27D4EB4Full;

struct OBArgs {
  uint64_t G, goff, stride;
  uint32_t R, S;
  uint32_t wide;         // the masks are 16-bit words
  uint32_t max_entries;
  uint64_t nb;           // chunks
  const void *sent, *snap, *hb_sent;
  // qe_progress
  const uint64_t *committed, *last_index, *run_first, *run_term;
  const uint8_t *run_count;
  const uint64_t *next;
  const uint32_t *peer;
  const uint64_t *snap_src;  // snap_index, or first_index with snap_sub 1
  uint64_t snap_sub;
  // qe_outbox_in
  const uint64_t *index, *next_before, *term, *snap_term, *hb_commit;
  const uint32_t *hb_ctx;
  // qe_outbox_out
  uint64_t cap;
  uint64_t *o_group;
  uint8_t *o_to, *o_type;
  uint64_t *o_term, *o_index, *o_log_term, *o_commit;
  uint32_t *o_ctx, *o_ent_len;
  uint64_t *o_ent_term;
  // scratch
  const uint64_t *offsets;
  uint32_t *counts;
  uint64_t *stats;
};

// defined in qe_inst_outbox.hip
int dispatch_outbox_count(const OBArgs &a, hipStream_t st);
int dispatch_outbox_fill(const OBArgs &a, uint32_t msg_runs, hipStream_t st);

// The counts of the layer: the three masks of a thread's groups, the rounds'
// loads independent and in flight together.  `wide`: the masks are 16-bit words.
struct OutboxCounts {
  const OBArgs &a;
  bool wide;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const uint32_t sz = wide ? 2u : 1u, full = (1u << a.S) - 1u;
    const rsrc_t rs = list_mask_rsrc(a.sent, base, nc, sz),
                 rp = list_mask_rsrc(a.snap, base, nc, sz),
                 rh = list_mask_rsrc(a.hb_sent, base, nc, sz);
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) {
      const uint32_t i = list_elem(r);
      k[r] = popc((list_ld_mask(rs, i, wide) | list_ld_mask(rp, i, wide) |
                   list_ld_mask(rh, i, wide)) & full);
    }
  }
};

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_outbox_count(OBArgs a) {
  list_count_block(a.G, a.counts, OutboxCounts{a, WIDE});
}

enum { O_GROUPS, O_APP, O_SNAP, O_HB, O_BAD, O_VIOL, O_ENTRIES, O_CSUM, O_N };

// Tile t, whose first record has position tb.
template <int RM, int E>
__device__ __forceinline__ void outbox_tile(const OBArgs &a, uint64_t t, uint64_t tb,
                                            uint32_t lane, uint64_t (&cnt)[O_N]) {
  const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
  const uint32_t sz = a.wide ? 2u : 1u, full = (1u << a.S) - 1u;
  // ---- 1. the masks: who sends what ----
  const uint32_t ms = list_ld_mask(list_mask_rsrc(a.sent, g0, n, sz), lane, a.wide) & full;
  const uint32_t mp = list_ld_mask(list_mask_rsrc(a.snap, g0, n, sz), lane, a.wide) & full;
  const uint32_t mb = list_ld_mask(list_mask_rsrc(a.hb_sent, g0, n, sz), lane, a.wide) & full;
  const uint32_t ma = ms & ~mp, mh = mb & ~(ms | mp);  // MsgSnap, then MsgApp, then MsgHeartbeat
  const uint32_t m = ma | mp | mh;
  const bool has = live && m != 0;
  const uint32_t u = wave_or(m);  // the tile's mask union (wave-uniform)
  // ---- 2. once per tile: term, the log, the snapshot, the heartbeat context ----
  const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), has ? o8 : kOOB);
  const bool need_a = ma != 0, need_s = mp != 0, need_h = mh != 0;
  const bool need_log = need_a || (need_s && !a.snap_term);
  uint64_t rf[RM], rt[RM];
#pragma unroll
  for (int r = 0; r < RM; r++) {
    rf[r] = 0;
    rt[r] = 0;
  }
  uint64_t li = 0, committed = 0;
  uint32_t nr = 0;
  if (__builtin_amdgcn_ballot_w64(need_log)) {
    const uint32_t l8 = need_log ? o8 : kOOB;
    li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), l8);
    committed = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), need_a ? o8 : kOOB);
    nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), need_log ? lane : kOOB);
    nr = nr < a.R ? nr : a.R;
#pragma unroll
    for (int r = 0; r < RM; r++)
      if (static_cast<uint32_t>(r) < a.R) {
        const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
        rf[r] = bld64<kNT>(mk_rsrc(a.run_first + row, n * 8), l8);
        rt[r] = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), l8);
      }
  }
  uint64_t sidx = 0, sterm = 0;
  if (__builtin_amdgcn_ballot_w64(need_s)) {
    const uint32_t s8 = need_s ? o8 : kOOB;
    sidx = bld64<kNT>(opt_rsrc(a.snap_src, g0, n), s8) - a.snap_sub;
    sterm = a.snap_term ? bld64<kNT>(mk_rsrc(a.snap_term + g0, n * 8), s8)
                        : run_term_at<RM>(rf, rt, nr, li, sidx);
  }
  uint32_t hctx = 0;
  if (__builtin_amdgcn_ballot_w64(need_h))
    hctx = bld32<kNT>(opt_rsrc(a.hb_ctx, g0, n), need_h ? lane * 4 : kOOB);
  // ---- 3. the per-slot rows of every slot in the union: m.Index of a MsgApp,
  // Commit of a MsgHeartbeat ----
  uint64_t v[QE_MAX_SLOTS];
#pragma unroll
  for (int s = 0; s < QE_MAX_SLOTS; s++) {
    v[s] = 0;
    if ((u >> s) & 1u) {
      const uint64_t row = static_cast<uint64_t>(s) * a.stride + g0;
      const bool ab = (ma >> s) & 1u, hb = (mh >> s) & 1u;
      uint64_t x = 0;
      if (a.index) {
        x = bld64<kNT>(mk_rsrc(a.index + row, n * 8), ab ? o8 : kOOB);
      } else if (a.next_before && __builtin_amdgcn_ballot_w64(ab)) {
        // Next - 1: from before the call where the peer replicates now
        const uint32_t pw = bld32<kNT>(mk_rsrc(a.peer + row, n * 4), ab ? lane * 4 : kOOB);
        const bool repl = (pw & QE_PF_STATE) == QE_PR_REPLICATE;
        x = (bld64<kNT>(mk_rsrc(a.next_before + row, n * 8), (ab && repl) ? o8 : kOOB) |
             bld64<kNT>(mk_rsrc(a.next + row, n * 8), (ab && !repl) ? o8 : kOOB)) -
            1u;
      }
      const uint64_t y = bld64<kNT>(opt_rsrc(a.hb_commit, row, n), hb ? o8 : kOOB);
      v[s] = ab ? x : y;
    }
  }
  // ---- 4. the records, slot by slot ----
  // what of the arrays this tile may write: capacity is the descriptors'
  const auto [tbc, rem] = list_room(tb, a.cap, kObTileMax);
  const rsrc_t d_group = mk_rsrc(a.o_group + tbc, rem * 8), d_to = mk_rsrc(a.o_to + tbc, rem),
               d_type = mk_rsrc(a.o_type + tbc, rem), d_term = mk_rsrc(a.o_term + tbc, rem * 8),
               d_index = mk_rsrc(a.o_index + tbc, rem * 8),
               d_lterm = mk_rsrc(a.o_log_term + tbc, rem * 8),
               d_commit = mk_rsrc(a.o_commit + tbc, rem * 8),
               d_ctx = a.o_ctx ? mk_rsrc(a.o_ctx + tbc, rem * 4) : mk_rsrc(a.o_ctx, 0);
  const uint64_t lim = a.max_entries ? a.max_entries : 0xFFFFFFFFull;
  uint32_t pbase = 0;
#pragma unroll
  for (int s = 0; s < QE_MAX_SLOTS; s++) {
    if (!((u >> s) & 1u)) continue;
    const bool bit = (m >> s) & 1u;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
    const uint32_t pos = pbase + lane_rank(bal);
    pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
    const bool is_s = (mp >> s) & 1u, is_a = (ma >> s) & 1u, is_h = (mh >> s) & 1u;
    // MsgApp: LogTerm and the entries (i, hi] cut into the table's runs
    const uint64_t i = v[s];
    const bool bad = is_a && (nr == 0 || i < rf[0] || i > li);
    const bool app = is_a && !bad;
    const uint64_t hi = li - i > lim ? i + lim : li;
    // run_cut of qe_step.hpp, written out: as a call, in any of the forms tried
    // (arrays by reference, a struct by value, forced or left to the inliner), it
    // costs every fill with entry runs 12-27 VGPRs at log_runs <= 8, with two
    // waves per SIMD before and after; whether that costs time was not settled
    // (DESIGN.md §6), so the registers decided
    uint32_t el[E > 0 ? E : 1] = {};
    uint64_t et[E > 0 ? E : 1] = {};
    uint32_t j = 0, ents = 0;
    if constexpr (E > 0) {
#pragma unroll
      for (int r = 0; r < RM; r++) {
        const uint64_t end = (r + 1 < RM && static_cast<uint32_t>(r + 1) < nr) ? rf[r + 1] - 1 : li;
        const uint64_t lo = rf[r] > i ? rf[r] : i + 1, e = end < hi ? end : hi;
        const bool ne = app && static_cast<uint32_t>(r) < nr && i < hi && lo <= e;
        const uint32_t len = static_cast<uint32_t>(e) - static_cast<uint32_t>(lo) + 1u;
#pragma unroll
        for (int k = 0; k < E; k++) {
          const bool sel = ne && j == static_cast<uint32_t>(k);
          el[k] = sel ? len : el[k];
          et[k] = sel ? rt[r] : et[k];
        }
        ents += (ne && j < static_cast<uint32_t>(E)) ? len : 0u;
        j += ne ? 1u : 0u;
      }
    }
    const uint32_t type =
        is_s ? QE_OMSG_SNAP : (bad ? QE_OMSG_BAD : (is_a ? QE_OMSG_APP : QE_OMSG_HEARTBEAT));
    const uint64_t idx = is_s ? sidx : (is_a ? i : 0);
    const uint64_t lt = is_s ? sterm : (app ? run_term_at<RM>(rf, rt, nr, li, i) : 0);
    const uint64_t cm = app ? committed : (is_h ? v[s] : 0);
    const uint32_t cx = is_h ? hctx : 0u;
    const uint32_t p1 = bit ? pos : kOOB, p4 = bit ? pos * 4 : kOOB, p8 = bit ? pos * 8 : kOOB;
    bst64<kNT>(gid, d_group, p8);
    bst8<kNT>(static_cast<uint32_t>(s), d_to, p1);
    bst8<kNT>(type, d_type, p1);
    bst64<kNT>(term, d_term, p8);
    bst64<kNT>(idx, d_index, p8);
    bst64<kNT>(lt, d_lterm, p8);
    bst64<kNT>(cm, d_commit, p8);
    bst32<kNT>(cx, d_ctx, p4);
    if constexpr (E > 0) {
#pragma unroll
      for (int k = 0; k < E; k++) {
        const uint64_t row = static_cast<uint64_t>(k) * a.cap + tbc;
        bst32<kNT>(el[k], mk_rsrc(a.o_ent_len + row, rem * 4), p4);
        bst64<kNT>(et[k], mk_rsrc(a.o_ent_term + row, rem * 8), p8);
      }
    }
    if (a.stats) {
      uint64_t h = mix64((gid * kPhi) ^ kOutboxSalt ^ (static_cast<uint64_t>(type) << 56) ^
                         (static_cast<uint64_t>(s) << 48));
      h = mix64(h ^ idx);
      h = mix64(h ^ lt);
      h = mix64(h ^ cm);
      h = mix64(h ^ ents);
      cnt[O_APP] += app ? 1u : 0u;
      cnt[O_SNAP] += is_s ? 1u : 0u;
      cnt[O_HB] += is_h ? 1u : 0u;
      cnt[O_BAD] += bad ? 1u : 0u;
      cnt[O_VIOL] += bad ? 1u : 0u;
      cnt[O_ENTRIES] += ents;
      cnt[O_CSUM] += bit ? h : 0u;
    }
  }
  cnt[O_GROUPS] += has ? 1u : 0u;
}

template <int RM, int E>
__global__ __launch_bounds__(kBlock) void k_outbox_fill(OBArgs a) {
  const int idx[O_N] = {QE_STAT_GROUPS,         QE_STAT_OUTBOX_APP,
                        QE_STAT_OUTBOX_SNAP,    QE_STAT_OUTBOX_HEARTBEAT,
                        QE_STAT_OUTBOX_BAD,     QE_STAT_INVARIANT_VIOLATIONS,
                        QE_STAT_OUTBOX_ENTRIES, QE_STAT_CHECKSUM};
  list_fill_walk<outbox_tile<RM, E>>(a, idx, OutboxCounts{a, a.wide != 0});
}

}  // namespace qe
