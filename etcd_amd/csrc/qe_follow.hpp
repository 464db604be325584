// qe_follow.hpp — qe_follower_step: the receiving side of MsgApp and
// MsgHeartbeat over the resident state.  The term preamble of raft.Step
// (raft/raft.go:847-920), becomeFollower (:686-693), handleAppendEntries and
// handleHeartbeat (:1475-1516) with raftLog.maybeAppend / findConflict /
// findConflictByTerm / commitTo (raft/log.go:88-168, :233-241) on the term-run
// log model, one message per group (include/etcd_quorum.h states the rules).
//
// The house idiom (qe_step.hpp).  Per tile:
//   1. type (1 B): which lanes have a message (a tile with none ends here);
//   2. for those lanes: from, m.Term, r.Term, state, m.Commit, committed,
//      last_index; for the MsgApp lanes m.Index, m.LogTerm and the E entry
//      runs -> the preamble and the stale check;
//   3. only when some lane has a MsgApp that is not stale: run_count and the
//      R run rows, held in registers.  term(), findConflict, the reject hint
//      and the truncate-and-append are closed forms over runs, unrolled at
//      compile time: no per-entry loop, no LDS;
//   4. the stores, each under the ballot of the lanes that changed the row: a
//      run row is stored only when some lane wrote it, so the common case (a
//      same-term append at the tail) stores no run row and no run_count.
//
// RM is the run-capacity bucket (log_runs <= 4 / 8 / 16), ENT whether the
// launch carries entries (msg_runs > 0): without them findConflict and the
// append are compiled out, and a heartbeat-only launch never reaches step 3.
// Its own argument struct: PArgs and every other kernel's code object are
// untouched.  The slot count is a run-time bound on `from` only, so the
// kernel is compiled once, not per QE_S.
#pragma once
#include "qe_step.hpp"

namespace qe {

struct FArgs {
  uint64_t G, goff, stride;
  uint32_t R, E, S, flags;
  // the log (qe_progress)
  uint64_t *committed, *last_index, *run_first, *run_term;
  uint8_t *run_count, *transferee;
  // qe_follower
  uint64_t *term;
  uint8_t *state, *lead, *vote;
  // qe_leader_msgs
  const uint8_t *type, *from;
  const uint64_t *mterm, *index, *log_term, *commit;
  const uint32_t *ent_len;
  const uint64_t *ent_term;
  // qe_follower_out
  uint8_t *result;
  uint64_t *resp_index, *reject_hint, *resp_log_term, *append_from;
  uint8_t *events;
  uint64_t *stats;
};

// defined in qe_inst_follow.hip
int dispatch_follow(const FArgs &a, hipStream_t st);

constexpr uint64_t kFollowSalt = 0x2545F4914F6CDD1Dull;
constexpr int kMsgRuns = QE_MAX_MSG_RUNS;

enum { F_GROUPS, F_ACCEPT, F_REJECT, F_APPENDED, F_ADV, F_REFUSED, F_CSUM, F_N };

template <int RM, bool ENT>
__global__ __launch_bounds__(kBlock) void k_follow(FArgs a) {
  uint64_t cnt[F_N] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  const bool resp_low = a.flags != 0;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
    // ---- 1. who has a message ----
    const uint32_t ty = msg_type(a.type, g0, n, lane);
    const bool has = live && ty != QE_LMSG_NONE;
    uint32_t res = QE_FR_NONE, ev = 0;
    if (__builtin_amdgcn_ballot_w64(has)) {
      // ---- 2. the message and the group's header ----
      const uint32_t h1 = has ? lane : kOOB, h8 = has ? o8 : kOOB;
      const bool isapp = has && ty == QE_LMSG_APP, ishb = has && ty == QE_LMSG_HEARTBEAT;
      const uint32_t from = bld8<kNT>(mk_rsrc(a.from + g0, n), h1);
      const uint64_t mterm = bld64<kNT>(mk_rsrc(a.mterm + g0, n * 8), h8);
      const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), h8);
      const uint32_t st = bld8<kNT>(mk_rsrc(a.state + g0, n), h1);
      const uint64_t mcommit = bld64<kNT>(mk_rsrc(a.commit + g0, n * 8), h8);
      const uint64_t committed = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), h8);
      const uint64_t li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), h8);
      uint64_t index = 0, log_term = 0;
      uint32_t len[kMsgRuns];
      uint64_t et[kMsgRuns];
#pragma unroll
      for (int j = 0; j < kMsgRuns; j++) {
        len[j] = 0;
        et[j] = 0;
      }
      if (__builtin_amdgcn_ballot_w64(isapp)) {
        const uint32_t a8 = isapp ? o8 : kOOB;
        index = bld64<kNT>(mk_rsrc(a.index + g0, n * 8), a8);
        log_term = bld64<kNT>(mk_rsrc(a.log_term + g0, n * 8), a8);
        if constexpr (ENT) {
#pragma unroll
          for (int j = 0; j < kMsgRuns; j++) {
            if (static_cast<uint32_t>(j) < a.E) {
              const uint64_t row = static_cast<uint64_t>(j) * a.stride + g0;
              len[j] = bld32<kNT>(mk_rsrc(a.ent_len + row, n * 4), isapp ? lane * 4 : kOOB);
              et[j] = bld64<kNT>(mk_rsrc(a.ent_term + row, n * 8), a8);
            }
          }
        }
      }
      // ---- the input checks and the term preamble ----
      bool bad = has && (ty > QE_LMSG_HEARTBEAT || from >= a.S);
      uint64_t nent = 0, prev = 0;
#pragma unroll
      for (int j = 0; j < kMsgRuns; j++) {
        const bool on = len[j] != 0;
        bad = bad || (on && (et[j] == 0 || et[j] < prev));
        prev = on ? et[j] : prev;
        nent += len[j];
      }
      const uint64_t lastnew = index + nent;
      // 2^64 - 1 is no log index (the ci = kInf below, li + 1, Next on the leader's side)
      bad = bad || lastnew < index || lastnew == kInf;
      const bool lower = mterm < term, higher = mterm > term;
      const bool lead_same = !lower && !higher && st == QE_STATE_LEADER;
      const bool proceed = has && !bad && !lower && !lead_same;
      // becomeFollower(m.Term, from)
      const bool bf =
          proceed && (higher || st == QE_STATE_CANDIDATE || st == QE_STATE_PRE_CANDIDATE);
      const bool app = proceed && isapp, hb = proceed && ishb;
      const bool stale = app && index < committed;
      const bool need = app && !stale;
      // ---- 3. the run table, when some MsgApp of the tile reaches the log ----
      uint64_t rf[RM], rt[RM];
#pragma unroll
      for (int r = 0; r < RM; r++) {
        rf[r] = 0;
        rt[r] = 0;
      }
      uint32_t nr = 0;
      if (__builtin_amdgcn_ballot_w64(need)) {
        const uint32_t n8 = need ? o8 : kOOB;
        nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), need ? lane : kOOB);
        nr = nr < a.R ? nr : a.R;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (static_cast<uint32_t>(r) < a.R) {
            const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
            rf[r] = bld64<kNT>(mk_rsrc(a.run_first + row, n * 8), n8);
            rt[r] = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), n8);
          }
        }
      }
      // matchTerm(m.Index, m.LogTerm); the hint of a rejection (:1496-1498)
      const bool match = run_term_at<RM>(rf, rt, nr, li, index) == log_term;
      const bool rej = need && !match, acc = need && match;
      const uint64_t hint =
          find_conflict_by_term<RM>(rf, rt, nr, li, index < li ? index : li, log_term);
      const uint64_t hterm = run_term_at<RM>(rf, rt, nr, li, hint);
      // findConflict: the first index of a message run where a log run of
      // another term overlaps it, or the first index past last_index
      uint64_t ci = kInf;
      uint32_t ncnt = nr, chg = 0;
      bool full = false, trunc = false, gap = false, confc = false;
      if constexpr (ENT) {
        uint64_t s = index + 1;
#pragma unroll
        for (int j = 0; j < kMsgRuns; j++) {
          const bool on = len[j] != 0;
          const uint64_t e = s + len[j] - 1;
#pragma unroll
          for (int r = 0; r < RM; r++) {
            // the run's last index
            const int r1 = r + 1 < RM ? r + 1 : r;
            const uint64_t b = (r + 1 < RM && static_cast<uint32_t>(r + 1) < nr) ? rf[r1] - 1 : li;
            const uint64_t lo = s > rf[r] ? s : rf[r], hi = e < b ? e : b;
            const bool diff = on && static_cast<uint32_t>(r) < nr && rt[r] != et[j] && lo <= hi;
            ci = (diff && lo < ci) ? lo : ci;
          }
          const uint64_t past = s > li + 1 ? s : li + 1;
          ci = (on && e > li && past < ci) ? past : ci;
          s += len[j];
        }
        const bool has_ci = acc && ci != kInf;
        gap = has_ci && ci > li + 1;
        confc = has_ci && ci <= committed;
        trunc = has_ci && !gap && !confc;
        // truncateAndAppend on runs: keep the runs that start below ci, then
        // the message's pieces from ci on
        uint32_t keep = 0;
        uint64_t last_t = 0;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          const bool k = static_cast<uint32_t>(r) < nr && rf[r] < ci;
          keep += k ? 1u : 0u;
          last_t = k ? rt[r] : last_t;
        }
        ncnt = trunc ? keep : nr;
        s = index + 1;
#pragma unroll
        for (int j = 0; j < kMsgRuns; j++) {
          const uint64_t e = s + len[j] - 1;
          const uint64_t ps = s > ci ? s : ci;
          const bool piece = trunc && len[j] != 0 && ps <= e;
          const bool row = piece && et[j] != last_t;
          full = full || (row && ncnt >= a.R);
#pragma unroll
          for (int r = 0; r < RM; r++) {
            const bool w = row && ncnt == static_cast<uint32_t>(r);
            rf[r] = w ? ps : rf[r];
            rt[r] = w ? et[j] : rt[r];
            chg |= w ? (1u << r) : 0u;
          }
          ncnt += row ? 1u : 0u;
          last_t = piece ? et[j] : last_t;
          s += len[j];
        }
      }
      const uint64_t new_li = trunc ? lastnew : li;
      // commitTo: min(m.Commit, lastnewi) for an append, m.Commit for a beat
      const uint64_t tc = (acc && lastnew < mcommit) ? lastnew : mcommit;
      const bool commits = acc || hb;
      const bool past_log = commits && tc > new_li;
      const uint64_t new_c = (commits && tc > committed) ? tc : committed;
      // ---- the result ----
      uint64_t ridx = 0;
      res = lower ? (resp_low ? QE_FR_LOWER_TERM_RESP : QE_FR_IGNORED) : QE_FR_IGNORED;
      res = hb ? QE_FR_HEARTBEAT_RESP : res;
      res = stale ? QE_FR_APP_STALE : res;
      res = rej ? QE_FR_APP_REJECT : res;
      res = acc ? QE_FR_APP_ACCEPT : res;
      res = past_log ? QE_FR_COMMIT_PAST_LOG : res;
      res = (trunc && full) ? QE_FR_RUNS_FULL : res;
      res = confc ? QE_FR_CONFLICT_COMMITTED : res;
      res = gap ? QE_FR_APP_GAP : res;
      res = bad ? QE_FR_BAD_MSG : res;
      res = has ? res : QE_FR_NONE;
      ridx = stale ? committed : ridx;
      ridx = rej ? index : ridx;
      ridx = acc ? lastnew : ridx;
      const bool refused = res >= QE_FR_REFUSED;
      const bool ok = proceed && !refused;
      const bool okbf = bf && !refused;
      ev = ok ? (bf ? QE_TEV_RESET : QE_TEV_HEARD) : 0u;
      const bool w_app = trunc && ok;
      const bool w_commit = ok && new_c != committed;
      const bool w_resp = has && !refused;
      const bool w_rej = rej && ok;
      // ---- 4. the stores ----
      const bool w_term = okbf && higher;
      become_follower_stores(a, g0, n, lane, w_term, okbf, ok, mterm, st, from);
      if (__builtin_amdgcn_ballot_w64(w_commit))
        bst64<kNT>(new_c, mk_rsrc(a.committed + g0, n * 8), w_commit ? o8 : kOOB);
      if constexpr (ENT) {
        if (__builtin_amdgcn_ballot_w64(w_app)) {
          bst64<kNT>(new_li, mk_rsrc(a.last_index + g0, n * 8), w_app ? o8 : kOOB);
          const bool w_nr = w_app && ncnt != nr;
          if (__builtin_amdgcn_ballot_w64(w_nr))
            bst8<kNT>(ncnt, mk_rsrc(a.run_count + g0, n), w_nr ? lane : kOOB);
          const uint32_t rows = w_app ? chg : 0u;
#pragma unroll
          for (int r = 0; r < RM; r++) {
            if (static_cast<uint32_t>(r) < a.R && __builtin_amdgcn_ballot_w64((rows >> r) & 1u)) {
              const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
              bst64<kNT>(rf[r], mk_rsrc(a.run_first + row, n * 8), bit_off(rows, r, o8));
              bst64<kNT>(rt[r], mk_rsrc(a.run_term + row, n * 8), bit_off(rows, r, o8));
            }
          }
        }
      }
      if (__builtin_amdgcn_ballot_w64(w_resp)) {
        const uint32_t r8 = w_resp ? o8 : kOOB;
        bst64<kNT>(ridx, opt_rsrc(a.resp_index, g0, n), r8);
        bst64<kNT>(w_app ? ci : 0, opt_rsrc(a.append_from, g0, n), r8);
      }
      if (__builtin_amdgcn_ballot_w64(w_rej)) {
        bst64<kNT>(hint, opt_rsrc(a.reject_hint, g0, n), w_rej ? o8 : kOOB);
        bst64<kNT>(hterm, opt_rsrc(a.resp_log_term, g0, n), w_rej ? o8 : kOOB);
      }
      if (a.stats) {
        const uint64_t term_after = w_term ? mterm : term;
        const uint64_t c_after = w_commit ? new_c : committed;
        const uint64_t li_after = w_app ? new_li : li;
        uint64_t h = mix64((gid * kPhi) ^ kFollowSalt ^ (static_cast<uint64_t>(res) << 56));
        h = mix64(h ^ term_after);
        h = mix64(h ^ c_after);
        h = mix64(h ^ li_after);
        cnt[F_GROUPS] += has ? 1u : 0u;
        cnt[F_ACCEPT] += (has && res == QE_FR_APP_ACCEPT) ? 1u : 0u;
        cnt[F_REJECT] += (has && res == QE_FR_APP_REJECT) ? 1u : 0u;
        cnt[F_APPENDED] += w_app ? lastnew - ci + 1 : 0u;
        cnt[F_ADV] += w_commit ? 1u : 0u;
        cnt[F_REFUSED] += (has && refused) ? 1u : 0u;
        cnt[F_CSUM] += has ? h : 0u;
      }
    }
    st_result_events(a.result, a.events, g0, n, lane, res, ev);
  }
  if (a.stats) {
    const int idx[F_N] = {QE_STAT_GROUPS,          QE_STAT_GRANTED,
                          QE_STAT_REJECTED,        QE_STAT_FOLLOW_APPENDED,
                          QE_STAT_COMMIT_ADVANCED, QE_STAT_INVARIANT_VIOLATIONS,
                          QE_STAT_CHECKSUM};
    wave_stats_add<F_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
