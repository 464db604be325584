// qe_snap.hpp — the log's lower end on the resident state.
//
// k_compact (qe_compact): MemoryStorage.CreateSnapshot and MemoryStorage.Compact
// (raft/storage.go:194-236) on the term-run log: the snapshot's index and term
// are recorded, the runs below the compaction index are dropped and the dummy
// row moved up to it.
//
// k_snap (qe_snapshot_step): one MsgSnap per group through the term preamble of
// raft.Step (raft/raft.go:849-920), the MsgSnap arms of stepFollower /
// stepCandidate (:1396-1398, :1441-1444), handleSnapshot / restore
// (:1518-1614) with raftLog.restore (raft/log.go:333-337) and the result of
// confchange.Restore (raft/confchange/restore.go) in mask form
// (include/etcd_quorum.h states the rules of both).
//
// The house idiom (qe_step.hpp).
//
// k_snap per tile:
//   1. type (1 B): which lanes have a message (a tile with none ends here,
//      with its result and events rows stored);
//   2. for those lanes: from, m.Term, r.Term, state, the snapshot's index and
//      committed -> the preamble and the stale check;
//   3. for the lanes that reach restore(): self_slot, the ConfState masks,
//      the snapshot's term, last_index, run_count;
//   4. only when some member lane's snapshot index lies inside its log: the run
//      rows, one pass with no table in registers (matchTerm);
//   5. the stores; the slot ids of a restored group row by row.
// k_compact per tile: the two request rows; for the lanes with a request
// committed, last_index, applied, snap_index, run_count and the run_first
// rows; run_term only when some lane creates a snapshot or drops a run.  The
// table lives in registers and moves down by r* rows through a barrel shift
// (log2 RM select stages); with r* == 0 one run_first word is stored.
//
// MT is the mask type (u8 for up to 8 slots, u16 above); RM the run-capacity
// bucket of k_follow (log_runs <= 4 / 8 / 16).  The slot count is a run-time
// value, so the object is compiled once, not per QE_S.  Own argument structs:
// no other kernel's code object changes.  No LDS, no scratch.
#pragma once
#include "qe_step.hpp"

namespace qe {

struct CPArgs {
  uint64_t G, goff, stride;
  uint32_t R, pad;
  const uint64_t *committed, *last_index;
  uint64_t *run_first, *run_term;
  uint8_t *run_count;
  uint64_t *first_index, *snap_index;
  const uint64_t *compact_index, *create_index, *applied;
  uint64_t *snap_term;
  uint8_t *result;
  uint64_t *stats;
};

struct SNArgs {
  uint64_t G, goff, stride;
  uint32_t R, S;
  // the log (qe_progress)
  uint64_t *committed, *last_index, *run_first, *run_term;
  uint8_t *run_count;
  uint64_t *first_index, *snap_index;
  const uint8_t *self_slot;
  uint8_t *transferee;
  // qe_follower
  uint64_t *term;
  uint8_t *state, *lead, *vote;
  // qe_conf
  uint64_t *slot_ids;
  void *c_inc, *c_out, *c_lrn, *c_lnx, *c_isl, *c_trk;
  uint8_t *c_auto;
  // qe_snap_msgs
  const uint8_t *type, *from;
  const uint64_t *mterm, *sindex, *sterm;
  const void *m_inc, *m_out, *m_lrn, *m_lnx;
  const uint8_t *m_auto;
  const uint64_t *m_ids;
  // qe_snap_out
  uint8_t *result;
  uint64_t *resp_index;
  uint8_t *events;
  uint64_t *stats;
};

// defined in qe_inst_snap.hip
int dispatch_compact(const CPArgs &a, hipStream_t st);
int dispatch_snap(const SNArgs &a, hipStream_t st);

constexpr uint64_t kCompactSalt = 0xD1B54A32D192ED03ull;
constexpr uint64_t kSnapSalt = 0x8CB92BA72F3D8DD7ull;

enum { K_GROUPS, K_ENTRIES, K_REFUSED, K_CSUM, K_N };

template <int RM>
__global__ __launch_bounds__(kBlock) void k_compact(CPArgs a) {
  uint64_t cnt[K_N] = {0, 0, 0, 0};
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
    // ---- 1. who has a request ----
    const uint64_t ci = bld64<kNT>(mk_rsrc(a.compact_index + g0, n * 8), o8);
    const uint64_t si = bld64<kNT>(opt_rsrc(a.create_index, g0, n), o8);
    const bool has = live && (ci | si) != 0;
    uint32_t res = QE_CP_NONE;
    if (__builtin_amdgcn_ballot_w64(has)) {
      // ---- 2. the log's header and the run starts ----
      const uint32_t h1 = has ? lane : kOOB, h8 = has ? o8 : kOOB;
      const bool c_on = has && si != 0, k_on = has && ci != 0;
      const uint64_t committed = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), h8);
      const uint64_t li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), h8);
      const uint64_t applied = a.applied ? bld64<kNT>(mk_rsrc(a.applied + g0, n * 8), h8) : kInf;
      const bool ld_snap = a.stats ? has : c_on;
      uint64_t snap = 0;
      if (__builtin_amdgcn_ballot_w64(ld_snap))
        snap = bld64<kNT>(opt_rsrc(a.snap_index, g0, n), ld_snap ? o8 : kOOB);
      uint32_t nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), h1);
      nr = nr < a.R ? nr : a.R;
      uint64_t rf[RM], rt[RM];
#pragma unroll
      for (int r = 0; r < RM; r++) {
        rf[r] = 0;
        rt[r] = 0;
        if (static_cast<uint32_t>(r) < a.R)
          rf[r] = bld64<kNT>(mk_rsrc(a.run_first + static_cast<uint64_t>(r) * a.stride + g0, n * 8),
                             h8);
      }
      // ---- decide ----
      const uint64_t d0 = rf[0];
      const uint64_t bound = applied < committed ? applied : committed;
      const bool c_ood = c_on && si <= snap;                        // ErrSnapOutOfDate
      const bool c_oob = c_on && !c_ood && (si > li || si < d0);    // the panic / slice bounds
      const bool c_pa = c_on && !c_ood && !c_oob && si > bound;
      const bool k_al = k_on && ci <= d0;                           // ErrCompacted
      const bool k_oob = k_on && !k_al && ci > li;
      const bool k_pa = k_on && !k_al && !k_oob && ci > bound;
      const bool refused = c_oob || c_pa || k_oob || k_pa;
      const bool c_ok = c_on && !c_ood && !refused;
      const bool k_ok = k_on && !k_al && !refused;
      // r*: the highest run that starts at or below ci (run 0 does: ci > d0)
      uint32_t below = 0;
#pragma unroll
      for (int r = 0; r < RM; r++)
        below += (static_cast<uint32_t>(r) < nr && rf[r] <= ci) ? 1u : 0u;
      const uint32_t rs = (k_ok && below) ? below - 1u : 0u;
      const bool shift = rs != 0;
      // ---- 3. the run terms, when a snapshot is created or a run dropped ----
      const bool need_rt = c_ok || shift;
      if (__builtin_amdgcn_ballot_w64(need_rt)) {
#pragma unroll
        for (int r = 0; r < RM; r++)
          if (static_cast<uint32_t>(r) < a.R)
            rt[r] = bld64<kNT>(mk_rsrc(a.run_term + static_cast<uint64_t>(r) * a.stride + g0, n * 8),
                               need_rt ? o8 : kOOB);
      }
      const uint64_t sterm = run_term_at<RM>(rf, rt, nr, li, si);
      // the table moves down by rs rows: a barrel shift, one stage per bit
#pragma unroll
      for (int b = 1; b < RM; b <<= 1) {
        const bool on = (rs & static_cast<uint32_t>(b)) != 0;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          const int q = r + b < RM ? r + b : r;
          rf[r] = (on && r + b < RM) ? rf[q] : rf[r];
          rt[r] = (on && r + b < RM) ? rt[q] : rt[r];
        }
      }
      const uint32_t ncnt = nr - rs;
      // ---- the result ----
      res = (c_ok ? QE_CP_CREATED : 0u) | (k_ok ? QE_CP_COMPACTED : 0u) |
            (c_ood ? QE_CP_SNAP_OUT_OF_DATE : 0u) | (k_al ? QE_CP_ALREADY : 0u);
      res = k_pa ? QE_CP_PAST_APPLIED : res;
      res = k_oob ? QE_CP_OUT_OF_BOUND : res;
      res = c_pa ? QE_CP_PAST_APPLIED : res;
      res = c_oob ? QE_CP_OUT_OF_BOUND : res;
      res = has ? res : QE_CP_NONE;
      // ---- 4. the stores ----
      if (__builtin_amdgcn_ballot_w64(c_ok)) {
        bst64<kNT>(si, opt_rsrc(a.snap_index, g0, n), c_ok ? o8 : kOOB);
        bst64<kNT>(sterm, opt_rsrc(a.snap_term, g0, n), c_ok ? o8 : kOOB);
      }
      if (__builtin_amdgcn_ballot_w64(k_ok)) {
        bst64<kNT>(ci, mk_rsrc(a.run_first + g0, n * 8), k_ok ? o8 : kOOB);
        bst64<kNT>(ci + 1, opt_rsrc(a.first_index, g0, n), k_ok ? o8 : kOOB);
      }
      if (__builtin_amdgcn_ballot_w64(shift)) {
        bst8<kNT>(ncnt, mk_rsrc(a.run_count + g0, n), shift ? lane : kOOB);
        bst64<kNT>(rt[0], mk_rsrc(a.run_term + g0, n * 8), shift ? o8 : kOOB);
#pragma unroll
        for (int r = 1; r < RM; r++) {
          const bool w = shift && static_cast<uint32_t>(r) < ncnt;
          if (static_cast<uint32_t>(r) < a.R && __builtin_amdgcn_ballot_w64(w)) {
            const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
            bst64<kNT>(rf[r], mk_rsrc(a.run_first + row, n * 8), w ? o8 : kOOB);
            bst64<kNT>(rt[r], mk_rsrc(a.run_term + row, n * 8), w ? o8 : kOOB);
          }
        }
      }
      if (a.stats) {
        uint64_t h = mix64((gid * kPhi) ^ kCompactSalt ^ (static_cast<uint64_t>(res) << 56));
        h = mix64(h ^ (k_ok ? ci : d0));
        h = mix64(h ^ ncnt);
        h = mix64(h ^ (c_ok ? si : snap));
        cnt[K_GROUPS] += has ? 1u : 0u;
        cnt[K_ENTRIES] += k_ok ? ci - d0 : 0u;
        cnt[K_REFUSED] += (has && refused) ? 1u : 0u;
        cnt[K_CSUM] += has ? h : 0u;
      }
    }
    bst8<kNT>(res, mk_rsrc(a.result + g0, n), lane);
  }
  if (a.stats) {
    const int idx[K_N] = {QE_STAT_GROUPS, QE_STAT_COMPACTED, QE_STAT_INVARIANT_VIOLATIONS,
                          QE_STAT_CHECKSUM};
    wave_stats_add<K_N>(cnt, idx, a.stats);
  }
}

enum { N_GROUPS, N_RESTORED, N_REJECT, N_ADV, N_REFUSED, N_CSUM, N_N };

template <typename MT>
__global__ __launch_bounds__(kBlock) void k_snap(SNArgs a) {
  uint64_t cnt[N_N] = {0, 0, 0, 0, 0, 0};
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  const uint32_t full = (1u << a.S) - 1u;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
    // ---- 1. who has a message ----
    const uint32_t ty = msg_type(a.type, g0, n, lane);
    const bool has = live && ty != QE_SMSG_NONE;
    uint32_t res = QE_SR_NONE, ev = 0;
    if (__builtin_amdgcn_ballot_w64(has)) {
      // ---- 2. the message's and the group's header ----
      const uint32_t h1 = has ? lane : kOOB, h8 = has ? o8 : kOOB;
      const uint32_t from = bld8<kNT>(mk_rsrc(a.from + g0, n), h1);
      const uint64_t mterm = bld64<kNT>(mk_rsrc(a.mterm + g0, n * 8), h8);
      const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), h8);
      const uint32_t st = bld8<kNT>(mk_rsrc(a.state + g0, n), h1);
      const uint64_t sindex = bld64<kNT>(mk_rsrc(a.sindex + g0, n * 8), h8);
      const uint64_t committed = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), h8);
      // 2^64 - 1 is no log index: first_index = sindex + 1 would wrap
      const bool bad = has && (ty != QE_SMSG_SNAP || from >= a.S || sindex == kInf);
      const bool lower = mterm < term, higher = mterm > term;
      const bool lead_same = !lower && !higher && st == QE_STATE_LEADER;
      const bool proceed = has && !bad && !lower && !lead_same;
      // becomeFollower(m.Term, from)
      const bool bf =
          proceed && (higher || st == QE_STATE_CANDIDATE || st == QE_STATE_PRE_CANDIDATE);
      const bool stale = proceed && sindex <= committed;
      const bool need = proceed && !stale;
      // ---- 3. the ConfState, the snapshot's term and the log's tail ----
      uint32_t self = 0xFFu, mi = 0, mo = 0, ml = 0, mn = 0, mauto = 0, nr = 0;
      uint64_t sterm = 0, li = 0;
      const bool ld_li = a.stats ? has : need;
      if (__builtin_amdgcn_ballot_w64(ld_li))
        li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), ld_li ? o8 : kOOB);
      if (__builtin_amdgcn_ballot_w64(need)) {
        const uint32_t n1 = need ? lane : kOOB;
        self = bld8<kNT>(mk_rsrc(a.self_slot + g0, n), n1);
        self = need ? self : 0xFFu;
        mi = ld_mask<MT, kNT>(mask_rsrc<MT>(a.m_inc, g0, n), lane, need);
        mo = ld_mask<MT, kNT>(mask_rsrc<MT>(a.m_out, g0, n), lane, need);
        ml = ld_mask<MT, kNT>(mask_rsrc<MT>(a.m_lrn, g0, n), lane, need);
        mn = ld_mask<MT, kNT>(mask_rsrc<MT>(a.m_lnx, g0, n), lane, need);
        mauto = bld8<kNT>(mk_rsrc(a.m_auto + g0, n), n1) != 0 ? 1u : 0u;
        sterm = bld64<kNT>(mk_rsrc(a.sterm + g0, n * 8), need ? o8 : kOOB);
        nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), n1);
        nr = nr < a.R ? nr : a.R;
      }
      const uint32_t selfb = self < a.S ? (1u << self) : 0u;
      const bool member = need && (selfb & (mi | ml | mo)) != 0;
      const bool notmem = need && !member;
      // ---- 4. term(sindex): the run rows, when the index is inside some log ----
      const bool inlog = member && sindex <= li;
      uint64_t lt = 0;
      if (__builtin_amdgcn_ballot_w64(inlog)) {
        uint64_t f0 = 0;
        for (uint32_t r = 0; r < a.R; r++) {
          const bool on = inlog && r < nr;
          if (__builtin_amdgcn_ballot_w64(on)) {
            const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
            const uint64_t f = bld64<kNT>(mk_rsrc(a.run_first + row, n * 8), on ? o8 : kOOB);
            const uint64_t v = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), on ? o8 : kOOB);
            f0 = r == 0 ? f : f0;
            lt = (on && sindex >= f) ? v : lt;
          }
        }
        lt = (nr == 0 || sindex < f0) ? 0 : lt;
      }
      // matchTerm(sindex, sterm): term() is 0 outside the log
      const bool match = member && lt == sterm;
      const bool past = match && sindex > li;
      const bool ff = match && !past;
      const bool torest = member && !match;
      const uint32_t allm = mi | mo | ml | mn;
      const bool badc =
          torest && ((mi == 0 && (mo | ml) != 0) || ((mi | mo) & ml) != 0 ||
                     (mn & ~(mo & ~mi)) != 0 || (mo == 0 && (mn != 0 || mauto != 0)) ||
                     (allm & ~full) != 0);
      const bool rest = torest && !badc;
      // ---- the result ----
      res = QE_SR_IGNORED;
      res = stale ? QE_SR_STALE : res;
      res = notmem ? QE_SR_NOT_MEMBER : res;
      res = ff ? QE_SR_FAST_FORWARD : res;
      res = rest ? QE_SR_RESTORED : res;
      res = past ? QE_SR_COMMIT_PAST_LOG : res;
      res = badc ? QE_SR_BAD_CONF : res;
      res = bad ? QE_SR_BAD_MSG : res;
      res = has ? res : QE_SR_NONE;
      const bool refused = res >= QE_SR_REFUSED;
      const bool ok = proceed && !refused;
      const bool okbf = bf && !refused;
      ev = ok ? (bf ? QE_TEV_RESET : QE_TEV_HEARD) : 0u;
      const bool w_commit = ff || rest;
      const bool w_resp = stale || notmem || ff || rest;
      const uint64_t ridx = (ff || rest) ? sindex : committed;
      // ---- 5. the stores ----
      const bool w_term = okbf && higher;
      become_follower_stores(a, g0, n, lane, w_term, okbf, ok, mterm, st, from);
      if (__builtin_amdgcn_ballot_w64(w_commit))
        bst64<kNT>(sindex, mk_rsrc(a.committed + g0, n * 8), w_commit ? o8 : kOOB);
      if (__builtin_amdgcn_ballot_w64(rest)) {
        const uint32_t r8 = rest ? o8 : kOOB, r1 = rest ? lane : kOOB;
        // raftLog.restore: the log is the snapshot's dummy entry alone
        bst64<kNT>(sindex, mk_rsrc(a.last_index + g0, n * 8), r8);
        bst64<kNT>(sindex, mk_rsrc(a.run_first + g0, n * 8), r8);
        bst64<kNT>(sterm, mk_rsrc(a.run_term + g0, n * 8), r8);
        bst8<kNT>(1u, mk_rsrc(a.run_count + g0, n), r1);
        bst64<kNT>(sindex + 1, opt_rsrc(a.first_index, g0, n), r8);
        bst64<kNT>(sindex, opt_rsrc(a.snap_index, g0, n), r8);
        // the tracker.Config confchange.Restore builds from the ConfState
        const uint32_t trk = mi | mo | ml;
        bst_mask<MT, kNT>(mi, mask_rsrc<MT>(a.c_inc, g0, n), lane, rest);
        bst_mask<MT, kNT>(mo, mask_rsrc<MT>(a.c_out, g0, n), lane, rest);
        bst_mask<MT, kNT>(ml, mask_rsrc<MT>(a.c_lrn, g0, n), lane, rest);
        bst_mask<MT, kNT>(mn, mask_rsrc<MT>(a.c_lnx, g0, n), lane, rest);
        bst_mask<MT, kNT>(ml, mask_rsrc<MT>(a.c_isl, g0, n), lane, rest);
        bst_mask<MT, kNT>(trk, mask_rsrc<MT>(a.c_trk, g0, n), lane, rest);
        bst8<kNT>(mauto, opt_rsrc(a.c_auto, g0, n), r1);
        if (a.slot_ids && a.m_ids) {
          for (uint32_t s = 0; s < a.S; s++) {
            const uint64_t id =
                bld64<kNT>(mk_rsrc(a.m_ids + static_cast<uint64_t>(s) * a.stride + g0, n * 8), r8);
            bst64<kNT>(((trk >> s) & 1u) ? id : 0,
                       mk_rsrc(a.slot_ids + static_cast<uint64_t>(s) * a.G + g0, n * 8), r8);
          }
        }
      }
      if (__builtin_amdgcn_ballot_w64(w_resp))
        bst64<kNT>(ridx, opt_rsrc(a.resp_index, g0, n), w_resp ? o8 : kOOB);
      if (a.stats) {
        uint64_t h = mix64((gid * kPhi) ^ kSnapSalt ^ (static_cast<uint64_t>(res) << 56));
        h = mix64(h ^ (w_term ? mterm : term));
        h = mix64(h ^ (w_commit ? sindex : committed));
        h = mix64(h ^ (rest ? sindex : li));
        cnt[N_GROUPS] += has ? 1u : 0u;
        cnt[N_RESTORED] += rest ? 1u : 0u;
        cnt[N_REJECT] += (stale || notmem) ? 1u : 0u;
        cnt[N_ADV] += w_commit ? 1u : 0u;
        cnt[N_REFUSED] += (has && refused) ? 1u : 0u;
        cnt[N_CSUM] += has ? h : 0u;
      }
    }
    st_result_events(a.result, a.events, g0, n, lane, res, ev);
  }
  if (a.stats) {
    const int idx[N_N] = {QE_STAT_GROUPS,          QE_STAT_GRANTED,
                          QE_STAT_REJECTED,        QE_STAT_COMMIT_ADVANCED,
                          QE_STAT_INVARIANT_VIOLATIONS, QE_STAT_CHECKSUM};
    wave_stats_add<N_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
