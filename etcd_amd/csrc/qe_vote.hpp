// qe_vote.hpp — qe_vote_step: elections over the resident state.  The term
// preamble of raft.Step for the vote messages with its lease check
// (raft/raft.go:849-920), the vote decision (:930-978), stepCandidate's
// response arm with RecordVote / TallyVotes (:1399-1414), hup / campaign
// (:760-835), MsgTimeoutNow (:1452-1457) and the header part of
// becomeFollower / becomePreCandidate / becomeCandidate / becomeLeader, one
// message per group (include/etcd_quorum.h states the rules).
//
// The house idiom (qe_step.hpp).  Per tile:
//   1. type (1 B): which lanes have a message (a tile with none ends here);
//   2. for those lanes: from, m.Term, the flags, r.Term, state, lead, vote;
//      m.Index and m.LogTerm for requests; in a candidate launch self_slot for
//      responses, MsgHup and MsgTimeoutNow;
//   3. in one round, each under its ballot: the timer for the higher-term
//      requests under CheckQuorum (the lease); last_index and run_count for
//      the requests that can vote and the lanes that may campaign; the Votes
//      and the configuration masks for responses and campaigns;
//   4. run_term of the last run: one row load per distinct run_count of the
//      tile's lanes that need the log (the one round trip that depends on a
//      loaded value; log_runs == 1 skips run_count);
//   5. the stores, each under the ballot of the lanes that changed the row.
//
// The lanes of step 3 are known before the lease is (the timer is in flight
// with the other rows), so they are a superset: a request that turns out to be
// in lease, and a pre-vote response that does not complete the quorum, have read
// the log rows without using them.
//
// MT is the mask type (u8 for up to 8 slots, u16 above), CAND whether the
// launch carries the Votes rows (voted / granted): without them the tally and
// the campaign are compiled out and responses, MsgHup and MsgTimeoutNow are
// refused.  The slot count is a run-time value (a bound and a mask clip), so
// the object is compiled once, not per QE_S.  Its own argument struct: no
// other kernel's code object changes.  No LDS, no scratch.
#pragma once
#include "qe_step.hpp"

namespace qe {

struct VArgs {
  uint64_t G, goff, stride;
  uint32_t R, S, et, flags;
  // qe_progress: the log's tail and the configuration, read only
  const uint64_t *last_index, *run_term;
  const uint8_t *run_count;
  const void *inc, *out, *tracked;
  const uint8_t *self_slot;
  uint8_t *transferee;
  // qe_follower
  uint64_t *term;
  uint8_t *state, *lead, *vote;
  // qe_voter
  const uint32_t *timer;
  void *voted, *granted;
  const uint8_t *no_campaign;
  // qe_vote_msgs
  const uint8_t *type, *from;
  const uint64_t *mterm, *index, *log_term;
  const uint8_t *mflags;
  // qe_vote_out
  uint8_t *result;
  uint64_t *resp_term, *req_log_term;
  void *req_to;
  uint8_t *elected, *events;
  uint64_t *stats;
};

// defined in qe_inst_vote.hip
int dispatch_vote(const VArgs &a, hipStream_t st);

constexpr uint64_t kVoteSalt = 0x9FB21C651E98DF25ull;

enum { V_GROUPS, V_GRANT, V_REJECT, V_PENDING, V_ELECT, V_LEADERS, V_DOWN, V_REFUSED, V_CSUM, V_N };

template <typename MT, bool CAND>
__global__ __launch_bounds__(kBlock) void k_vote(VArgs a) {
  uint64_t cnt[V_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  const uint32_t full = (1u << a.S) - 1u;
  const bool cq_on = (a.flags & QE_VOTE_CHECK_QUORUM) != 0;
  const bool pv_on = (a.flags & QE_VOTE_PREVOTE) != 0;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
    // ---- 1. who has a message ----
    const uint32_t ty = msg_type(a.type, g0, n, lane);
    const bool has = live && ty != QE_VMSG_NONE;
    uint32_t res = QE_VR_NONE, ev = 0, el = 0;
    if (__builtin_amdgcn_ballot_w64(has)) {
      // ---- 2. the message and the group's header ----
      const uint32_t h1 = has ? lane : kOOB, h8 = has ? o8 : kOOB;
      const uint32_t from = bld8<kNT>(mk_rsrc(a.from + g0, n), h1);
      const uint64_t mterm = bld64<kNT>(mk_rsrc(a.mterm + g0, n * 8), h8);
      const uint32_t mf = bld8<kNT>(opt_rsrc(a.mflags, g0, n), h1);
      const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), h8);
      const uint32_t st = bld8<kNT>(mk_rsrc(a.state + g0, n), h1);
      const uint32_t lead = bld8<kNT>(mk_rsrc(a.lead + g0, n), h1);
      const uint32_t vote = bld8<kNT>(mk_rsrc(a.vote + g0, n), h1);
      const bool isvote = has && ty == QE_VMSG_VOTE, isprev = has && ty == QE_VMSG_PREVOTE;
      const bool isvr = has && ty == QE_VMSG_VOTE_RESP, ispr = has && ty == QE_VMSG_PREVOTE_RESP;
      const bool ishup = has && ty == QE_VMSG_HUP, isto = has && ty == QE_VMSG_TIMEOUT_NOW;
      const bool isreq = isvote || isprev, isresp = isvr || ispr;
      const bool rej = (mf & QE_VMF_REJECT) != 0, force = (mf & QE_VMF_FORCE) != 0;
      uint64_t index = 0, log_term = 0;
      if (__builtin_amdgcn_ballot_w64(isreq)) {
        index = bld64<kNT>(mk_rsrc(a.index + g0, n * 8), isreq ? o8 : kOOB);
        log_term = bld64<kNT>(mk_rsrc(a.log_term + g0, n * 8), isreq ? o8 : kOOB);
      }
      uint32_t self = 0xFFu;
      bool bad = has && (ty > QE_VMSG_TIMEOUT_NOW || (!ishup && (from >= a.S || mterm == 0)));
      if constexpr (CAND) {
        const bool ns = isresp || ishup || isto;
        if (a.self_slot && __builtin_amdgcn_ballot_w64(ns)) {
          const uint32_t v = bld8<kNT>(mk_rsrc(a.self_slot + g0, n), ns ? lane : kOOB);
          self = ns ? v : 0xFFu;
        }
        bad = bad || (isresp && !a.self_slot) || ((ishup || isto) && self >= a.S);
      } else {
        bad = bad || isresp || ishup || isto;
      }
      const bool ok = has && !bad;
      // ---- the term preamble, as far as it is known without the timer ----
      const bool pre = ok && !ishup;
      const bool higher = pre && mterm > term, lower = pre && mterm < term;
      // MsgPreVote and a granted MsgPreVoteResp never change the term (:865-872)
      const bool nochange = isprev || (ispr && !rej);
      const bool bf_s = higher && !nochange;  // becomeFollower(m.term, None) unless in lease
      const uint32_t vote_s = bf_s ? 0xFFu : vote, lead_s = bf_s ? 0xFFu : lead;
      const bool canvote_s =
          ok && isreq && !lower &&
          (vote_s == from || (vote_s >= a.S && lead_s >= a.S) || (isprev && higher));
      const uint32_t st_s = bf_s ? static_cast<uint32_t>(QE_STATE_FOLLOWER) : st;
      bool mine = false, hupgo = false;
      if constexpr (CAND) {
        // stepCandidate's own response type; hup(): not a leader, and
        // MsgTimeoutNow reaches it on a follower only
        mine = ok && !lower &&
               ((isvr && st_s == QE_STATE_CANDIDATE) || (ispr && st_s == QE_STATE_PRE_CANDIDATE));
        hupgo = ok && !lower &&
                ((ishup && st_s != QE_STATE_LEADER) || (isto && st_s == QE_STATE_FOLLOWER));
      }
      // ---- 3. the rows by need ----
      const bool need_t = cq_on && higher && isreq;
      uint32_t ee = 0;
      if (__builtin_amdgcn_ballot_w64(need_t))
        ee = bld32<kNT>(mk_rsrc(a.timer + g0, n * 4), need_t ? lane * 4 : kOOB) & 0xFFFFu;
      const bool needlog = canvote_s || hupgo || (mine && ispr);
      uint64_t li = 0;
      uint32_t rc1 = 0;
      if (__builtin_amdgcn_ballot_w64(needlog)) {
        li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), needlog ? o8 : kOOB);
        if (a.R > 1)  // (a run_count of 0 matches no row: lastTerm 0)
          rc1 = bld8<kNT>(mk_rsrc(a.run_count + g0, n), needlog ? lane : kOOB) - 1u;
      }
      uint32_t mi = full, mo = 0, trk = full, vd = 0, gr = 0, nc = 0;
      if constexpr (CAND) {
        const bool needm = mine || hupgo;
        const bool ldv = needm || (a.stats && has);  // (the checksum covers the Votes)
        if (__builtin_amdgcn_ballot_w64(ldv)) {
          vd = ld_mask<MT, kNT>(mask_rsrc<MT>(a.voted, g0, n), lane, ldv);
          gr = ld_mask<MT, kNT>(mask_rsrc<MT>(a.granted, g0, n), lane, ldv);
        }
        if (__builtin_amdgcn_ballot_w64(needm)) {
          if (a.inc) mi = ld_mask<MT, kNT>(mask_rsrc<MT>(a.inc, g0, n), lane, needm) & full;
          if (a.out) mo = ld_mask<MT, kNT>(mask_rsrc<MT>(a.out, g0, n), lane, needm) & full;
        }
        if (__builtin_amdgcn_ballot_w64(hupgo)) {
          if (a.tracked)
            trk = ld_mask<MT, kNT>(mask_rsrc<MT>(a.tracked, g0, n), lane, hupgo) & full;
          nc = bld8<kNT>(opt_rsrc(a.no_campaign, g0, n), hupgo ? lane : kOOB);
        }
      }
      // ---- 4. lastTerm: run_term of the last run ----
      uint64_t lt = 0;
      if (__builtin_amdgcn_ballot_w64(needlog)) {
        for (uint32_t r = 0; r < a.R; r++) {
          const bool same = needlog && rc1 == r;
          if (__builtin_amdgcn_ballot_w64(same)) {
            const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
            const uint64_t v = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), same ? o8 : kOOB);
            lt = same ? v : lt;
          }
        }
      }
      // ---- decide ----
      // the lease (:852-862): nothing changes
      const bool inlease = need_t && !force && lead < a.S && ee < a.et;
      const bool bf = bf_s && !inlease;
      const uint64_t term1 = bf ? mterm : term;
      const uint32_t vote1 = bf ? 0xFFu : vote, lead1 = bf ? 0xFFu : lead;
      const uint32_t st1 = bf ? static_cast<uint32_t>(QE_STATE_FOLLOWER) : st;
      // requests (:930-978)
      const bool req = ok && isreq && !lower && !inlease;
      const bool utd = log_term > lt || (log_term == lt && index >= li);
      const bool grant = req && canvote_s && utd;
      const bool deny = (req && !grant) || (lower && isprev);
      const bool gvote = grant && isvote;
      // responses (:1399-1414), campaigns (:760-835)
      const uint32_t selfb = self < a.S ? (1u << self) : 0u;
      bool pend = false, lost = false, won = false, prec = false, cand = false, camp0 = false;
      bool rec = false;
      uint32_t vd2 = vd, gr2 = gr;
      if constexpr (CAND) {
        const uint32_t fb = 1u << (from & 15u);
        rec = mine && !(vd & fb);  // the first vote of `from` sticks
        const uint32_t vd1 = rec ? (vd | fb) : vd;
        const uint32_t gr1 = (rec && !rej) ? (gr | fb) : gr;
        const uint32_t tally = joint_vote(mi, mo, vd1, gr1);
        pend = mine && tally == kVotePending;
        lost = mine && tally == kVoteLost;
        const bool wonr = mine && tally == kVoteWon;
        const bool promotable = (selfb & trk & (mi | mo)) != 0;
        camp0 = hupgo && promotable && nc == 0;
        // the candidate's own vote decides a single-voter configuration
        const bool alone = joint_vote(mi, mo, selfb, selfb) == kVoteWon;
        prec = camp0 && ishup && pv_on;  // becomePreCandidate
        cand = (camp0 && !prec) || (prec && alone) || (wonr && ispr);  // becomeCandidate
        won = (cand && alone) || (wonr && isvr);
        // ResetVotes of 3d, then the campaign's own vote, then the reset of
        // becomeFollower (lost) / becomeLeader (won)
        vd2 = bf ? 0u : vd1;
        gr2 = bf ? 0u : gr1;
        vd2 = (cand || prec) ? selfb : vd2;
        gr2 = (cand || prec) ? selfb : gr2;
        vd2 = (lost || won) ? 0u : vd2;
        gr2 = (lost || won) ? 0u : gr2;
      }
      const bool precamp = prec && !cand, votecamp = cand && !won;
      const uint64_t term2 = cand ? term1 + 1 : term1;
      uint32_t vote2 = gvote ? from : vote1;
      vote2 = cand ? self : vote2;
      uint32_t st2 = lost ? static_cast<uint32_t>(QE_STATE_FOLLOWER) : st1;
      st2 = prec ? static_cast<uint32_t>(QE_STATE_PRE_CANDIDATE) : st2;
      st2 = cand ? static_cast<uint32_t>(QE_STATE_CANDIDATE) : st2;
      st2 = won ? static_cast<uint32_t>(QE_STATE_LEADER) : st2;
      uint32_t lead2 = (lost || prec || cand) ? 0xFFu : lead1;
      lead2 = won ? self : lead2;
      const bool reset = bf || lost || cand || won;
      ev = reset ? QE_TEV_RESET : (gvote ? QE_TEV_HEARD : 0u);
      el = won ? 1u : 0u;
      // ---- the result ----
      res = bf ? QE_VR_STEPPED_DOWN : QE_VR_IGNORED;
      res = inlease ? QE_VR_IN_LEASE : res;
      res = deny ? QE_VR_REJECT : res;
      res = grant ? QE_VR_GRANT : res;
      res = pend ? QE_VR_PENDING : res;
      res = lost ? QE_VR_LOST : res;
      res = precamp ? QE_VR_CAMPAIGN_PREVOTE : res;
      res = votecamp ? QE_VR_CAMPAIGN_VOTE : res;
      res = won ? QE_VR_WON : res;
      res = bad ? QE_VR_BAD_MSG : res;
      res = has ? res : QE_VR_NONE;
      uint64_t rterm = grant ? mterm : term1;  // a grant answers with the message's term
      rterm = precamp ? term1 + 1 : rterm;
      rterm = votecamp ? term2 : rterm;
      const bool w_req = precamp || votecamp;
      const bool w_resp = grant || deny || w_req;
      // ---- 5. the stores ----
      const bool w_term = term2 != term;
      if (__builtin_amdgcn_ballot_w64(w_term))
        bst64<kNT>(term2, mk_rsrc(a.term + g0, n * 8), w_term ? o8 : kOOB);
      const bool w_vote = vote2 != vote;
      if (__builtin_amdgcn_ballot_w64(w_vote))
        bst8<kNT>(vote2, mk_rsrc(a.vote + g0, n), w_vote ? lane : kOOB);
      const bool w_st = st2 != st;
      if (__builtin_amdgcn_ballot_w64(w_st))
        bst8<kNT>(st2, mk_rsrc(a.state + g0, n), w_st ? lane : kOOB);
      const bool w_lead = lead2 != lead;
      if (__builtin_amdgcn_ballot_w64(w_lead))
        bst8<kNT>(lead2, mk_rsrc(a.lead + g0, n), w_lead ? lane : kOOB);
      if (__builtin_amdgcn_ballot_w64(reset))
        bst8<kNT>(0xFFu, opt_rsrc(a.transferee, g0, n), reset ? lane : kOOB);
      if constexpr (CAND) {
        const bool w_m = bf || rec || lost || prec || cand || won;
        if (__builtin_amdgcn_ballot_w64(w_m)) {
          bst_mask<MT, kNT>(vd2, mask_rsrc<MT>(a.voted, g0, n), lane, w_m);
          bst_mask<MT, kNT>(gr2, mask_rsrc<MT>(a.granted, g0, n), lane, w_m);
        }
      }
      if (__builtin_amdgcn_ballot_w64(w_resp))
        bst64<kNT>(rterm, opt_rsrc(a.resp_term, g0, n), w_resp ? o8 : kOOB);
      if (__builtin_amdgcn_ballot_w64(w_req)) {
        bst64<kNT>(lt, opt_rsrc(a.req_log_term, g0, n), w_req ? o8 : kOOB);
        bst_mask<MT, kNT>((mi | mo) & ~selfb, mask_rsrc<MT>(a.req_to, g0, n), lane, w_req);
      }
      if (a.stats) {
        uint64_t h = mix64((gid * kPhi) ^ kVoteSalt ^ (static_cast<uint64_t>(res) << 56));
        h = mix64(h ^ term2);
        h = mix64(h ^ (st2 | (lead2 << 8) | (vote2 << 16) | (ev << 24)));
        h = mix64(h ^ (CAND ? (vd2 | (gr2 << 16)) : 0u));
        cnt[V_GROUPS] += has ? 1u : 0u;
        cnt[V_GRANT] += grant ? 1u : 0u;
        cnt[V_REJECT] += deny ? 1u : 0u;
        cnt[V_PENDING] += pend ? 1u : 0u;
        cnt[V_ELECT] += camp0 ? 1u : 0u;
        cnt[V_LEADERS] += won ? 1u : 0u;
        cnt[V_DOWN] += (bf ? 1u : 0u) + (lost ? 1u : 0u);
        cnt[V_REFUSED] += bad ? 1u : 0u;
        cnt[V_CSUM] += has ? h : 0u;
      }
    }
    st_result_events(a.result, a.events, g0, n, lane, res, ev);
    bst8<kNT>(el, opt_rsrc(a.elected, g0, n), lane);
  }
  if (a.stats) {
    const int idx[V_N] = {QE_STAT_GROUPS,    QE_STAT_GRANTED,   QE_STAT_REJECTED,
                          QE_STAT_VOTE_PENDING, QE_STAT_ELECTIONS, QE_STAT_LEADERS,
                          QE_STAT_STEPDOWNS, QE_STAT_INVARIANT_VIOLATIONS, QE_STAT_CHECKSUM};
    wave_stats_add<V_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
