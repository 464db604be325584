// qe_tick.hpp — qe_tick: raft.tick() over the resident state.  tickElection
// (raft/raft.go:645-654) on every group that does not lead, tickHeartbeat
// (:657-684) on every leader, with the MsgCheckQuorum (:997-1018) and the
// MsgBeat (bcastHeartbeat, :524-541) the timers fire executed in the same
// pass: with HeartbeatTick 1 every leader beats on every tick, so the tick is
// the heartbeat stream plus seven timer bytes per group.
//
// The house idiom (qe_step.hpp), as k_heartbeat / k_check_quorum
// (qe_progress.hpp).  Per tile:
//   1. the header: state (1 B), timer (4 B), randomizedElectionTimeout (2 B),
//      events (1 B) -> the timers and which of CheckQuorum / beat / campaign
//      fire (wave-wide ballots);
//   2. under those ballots, for the lanes that fired only: the masks, tracked,
//      self_slot, no_campaign, lead_transferee, committed, the queue head;
//   3. the tracked slots' peer words (CheckQuorum) and Match rows (beat);
//   4. every store, after every load of the tile (a buffer store orders the
//      loads after it, profiles/r06/heartbeat_ab2.txt).
// The timer row is stored whole; randomized_timeout whole when some lane drew
// again; state, lead_transferee and the peer-word rows only where a lane of
// the tile changed them.  Rows touched once per launch go non-temporal.
//
// Its own argument struct: PArgs (and with it every Progress kernel's code
// object) is untouched.  No LDS, no scratch: the statistics are wave sums
// added with one atomic per counter per wave (the grid is capped when
// statistics are asked for).
#pragma once
#include "qe_step.hpp"

namespace qe {

struct TArgs {
  uint64_t G, goff, stride;
  // qe_timers
  uint8_t *state;
  uint32_t *timer;
  uint16_t *rt;
  const uint8_t *no_campaign, *events;
  uint32_t et, ht, flags, ticks;
  uint64_t seed;
  uint32_t tick_no;
  // qe_progress
  uint32_t read_cap;
  uint32_t *pw;
  const uint64_t *match, *committed;
  const void *inc, *out, *tracked;
  const uint8_t *self_slot;
  uint8_t *transferee;
  const void *read_acks;
  const uint32_t *read_head;
  const uint8_t *read_count;
  // qe_tick_out
  uint8_t *action;
  uint64_t *hb_commit;
  uint32_t *hb_ctx;
  void *hb_sent;
  uint8_t *qactive;
  uint64_t *stats;
};

// defined in qe_inst_tick.hip and instantiated there for the object's QE_S
template <int S>
int dispatch_tick(const TArgs &a, bool masked, bool joint, hipStream_t st);

constexpr uint32_t kDrawStream = 0x7131;  // hash4 stream of the timeout draw
constexpr uint32_t kTimerMax = 0xFFFFu;   // the counters saturate here

// resetRandomizedElectionTimeout (raft/raft.go:1718-1720): electionTimeout +
// a uniform value of [0, electionTimeout), counter-based (the global group
// id and the host's tick number) where the reference draws from globalRand.
__device__ __forceinline__ uint32_t draw_timeout(const TArgs &a, uint64_t gid) {
  const uint64_t h = hash4(a.seed, gid, a.tick_no, kDrawStream);
  return a.et + static_cast<uint32_t>(((h >> 32) * a.et) >> 32);
}

enum { T_GROUPS, T_HUPS, T_STEPDOWNS, T_CSUM, T_N };

template <int S, typename MT, bool MASKED, bool JOINT>
__global__ __launch_bounds__(kBlock) void k_tick(TArgs a) {
  constexpr uint32_t kFull = (1u << S) - 1u;
  uint64_t cnt[T_N] = {0, 0, 0, 0};
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  const bool cq_on = (a.flags & QE_TICK_CHECK_QUORUM) != 0;
  const bool want_ctx = a.hb_ctx && a.read_acks;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
    const uint32_t o4 = lane * 4;
    // ---- 1. the header ----
    const uint32_t st0 = bld8<kNT>(mk_rsrc(a.state + g0, n), lane);
    const uint32_t tm0 = bld32<kNT>(mk_rsrc(a.timer + g0, n * 4), o4);
    uint32_t rt = bld16<kNT>(mk_rsrc(a.rt + g0, n * 2), lane * 2);
    const uint32_t ev = bld8<kNT>(opt_rsrc(a.events, g0, n), lane);
    uint32_t ee = tm0 & 0xFFFFu, he = tm0 >> 16;
    // events: the timer part of reset() (:597-599) wins over a plain
    // electionElapsed = 0
    const bool reset = live && (ev & QE_TEV_RESET) != 0;
    ee = (ev & (QE_TEV_RESET | QE_TEV_HEARD)) ? 0u : ee;
    he = reset ? 0u : he;
    if (__builtin_amdgcn_ballot_w64(reset)) rt = reset ? draw_timeout(a, gid) : rt;
    bool redraw = reset;
    uint32_t act = 0, state = st0, hb_to = 0, ctx = 0;
    if (a.ticks) {
      const bool leader = live && st0 == QE_STATE_LEADER;
      ee += ee < kTimerMax ? 1u : 0u;
      he += (leader && he < kTimerMax) ? 1u : 0u;
      // tickElection: past the timeout (promotable is decided below)
      const bool cand = live && !leader && ee >= rt;
      // tickHeartbeat: the election timeout elapsed on a leader
      const bool fire = leader && ee >= a.et;
      const bool cqf = fire && cq_on;
      const bool beatp = leader && he >= a.ht;  // (unless it steps down below)
      ee = fire ? 0u : ee;
      // ---- 2. what the lanes that fired need ----
      uint32_t mi = kFull, mo = 0, trk = kFull, self = 0xFFu, nc = 0, lt = 0xFFu;
      uint32_t qn = 0, qh = 0;
      uint64_t c = 0;
      const bool need = cand || cqf || beatp;
      if (__builtin_amdgcn_ballot_w64(need)) {
        if (a.tracked) trk = ld_slot_mask<MT, S>(a.tracked, g0, n, lane, need);
        if (a.self_slot) self = bld8<kNT>(mk_rsrc(a.self_slot + g0, n), need ? lane : kOOB);
      }
      if (__builtin_amdgcn_ballot_w64(cand || cqf)) {
        const bool on = cand || cqf;
        if constexpr (MASKED) mi = ld_slot_mask<MT, S>(a.inc, g0, n, lane, on);
        if constexpr (JOINT) mo = ld_slot_mask<MT, S>(a.out, g0, n, lane, on);
        nc = bld8<kNT>(opt_rsrc(a.no_campaign, g0, n), cand ? lane : kOOB);
      }
      if (a.transferee && __builtin_amdgcn_ballot_w64(fire))
        lt = bld8(mk_rsrc(a.transferee + g0, n), fire ? lane : kOOB);
      lt = fire ? lt : 0xFFu;
      if (__builtin_amdgcn_ballot_w64(beatp)) {
        if (a.hb_commit) c = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), beatp ? o8 : kOOB);
        if (want_ctx) {
          qn = bld8<kNT>(mk_rsrc(a.read_count + g0, n), beatp ? lane : kOOB);
          qh = bld32<kNT>(mk_rsrc(a.read_head + g0, n * 4), beatp ? o4 : kOOB);
        }
      }
      // ---- 3. the slot rows: peer words of the checked groups, Match of
      // the beating ones, all before the tile's first store ----
      const uint32_t selfb = self < static_cast<uint32_t>(S) ? (1u << self) : 0u;
      const uint32_t cq_trk = cqf ? trk : 0u;
      hb_to = beatp ? (trk & ~selfb) : 0u;
      uint32_t w[S];
      uint64_t m[S];
#pragma unroll
      for (int s = 0; s < S; s++) {
        w[s] = 0;
        m[s] = 0;
      }
      if (__builtin_amdgcn_ballot_w64(cqf)) {
#pragma unroll
        for (int s = 0; s < S; s++)
          w[s] = bld32(mk_rsrc(a.pw + static_cast<uint64_t>(s) * a.stride + g0, n * 4),
                       bit_off(cq_trk, s, o4));
      }
      if (a.hb_commit && __builtin_amdgcn_ballot_w64(beatp)) {
#pragma unroll
        for (int s = 0; s < S; s++)
          m[s] = bld64<kNT>(mk_rsrc(a.match + static_cast<uint64_t>(s) * a.stride + g0, n * 8),
                            bit_off(hb_to, s, o8));
      }
      // ---- decide ----
      // tickElection: promotable() (:1618-1621) and past the timeout -> MsgHup
      const bool promotable = ((selfb & trk & (mi | mo)) != 0) && nc == 0;
      const bool hup = cand && promotable;
      ee = hup ? 0u : ee;
      act |= hup ? QE_TICK_HUP : 0u;
      // MsgCheckQuorum as k_check_quorum decides it
      const uint32_t selft = selfb & trk;
      uint32_t ra = 0;
#pragma unroll
      for (int s = 0; s < S; s++) ra |= ((w[s] >> 3) & 1u) << s;
      ra = (ra & trk) | selft;
      const uint32_t present = (mi | mo) & trk;
      const bool qa = joint_vote(mi, mo, present, ra & present) == kVoteWon;
      const bool down = cqf && !qa;  // becomeFollower(r.Term, None)
      act |= cqf ? QE_TICK_CHECKED_QUORUM : 0u;
      act |= down ? QE_TICK_STEPDOWN : 0u;
      state = down ? static_cast<uint32_t>(QE_STATE_FOLLOWER) : state;
      ee = down ? 0u : ee;
      he = down ? 0u : he;
      if (__builtin_amdgcn_ballot_w64(down)) rt = down ? draw_timeout(a, gid) : rt;
      redraw = redraw || down;
      // the stepdown's reset() and abortLeaderTransfer (:669-671) both end a
      // transfer in progress
      const bool abort = fire && lt < static_cast<uint32_t>(S);
      act |= abort ? QE_TICK_TRANSFER_ABORTED : 0u;
      const bool beat = beatp && !down;
      he = beat ? 0u : he;
      act |= beat ? QE_TICK_BEAT : 0u;
      hb_to = beat ? hb_to : 0u;
      ctx = last_pending_ctx(qn, qh, a.read_cap);
      // ---- 4. the stores of what the timers fired ----
      if (__builtin_amdgcn_ballot_w64(cqf)) {
#pragma unroll
        for (int s = 0; s < S; s++) {
          const uint32_t nw =
              (w[s] & ~QE_PF_RECENT_ACTIVE) | (((selft >> s) & 1u) ? QE_PF_RECENT_ACTIVE : 0u);
          const bool wr = ((cq_trk >> s) & 1u) && nw != w[s];
          // a row some lane changes is stored for every tracked slot of the
          // checked lanes (whole sectors, as k_check_quorum)
          if (__builtin_amdgcn_ballot_w64(wr))
            bst32(nw, mk_rsrc(a.pw + static_cast<uint64_t>(s) * a.stride + g0, n * 4),
                  bit_off(cq_trk, s, o4));
        }
        if (a.qactive) bst8<kNT>(qa ? 1u : 0u, mk_rsrc(a.qactive + g0, n), cqf ? lane : kOOB);
      }
      if (__builtin_amdgcn_ballot_w64(down))
        bst8<kNT>(state, mk_rsrc(a.state + g0, n), down ? lane : kOOB);
      if (__builtin_amdgcn_ballot_w64(abort))
        bst8(0xFFu, mk_rsrc(a.transferee + g0, n), abort ? lane : kOOB);
      if (__builtin_amdgcn_ballot_w64(beat)) {
        if (a.hb_ctx) bst32<kNT>(ctx, mk_rsrc(a.hb_ctx + g0, n * 4), beat ? o4 : kOOB);
        if (a.hb_commit) {
#pragma unroll
          for (int s = 0; s < S; s++)
            bst64<kNT>(m[s] < c ? m[s] : c,
                       mk_rsrc(a.hb_commit + static_cast<uint64_t>(s) * a.stride + g0, n * 8),
                       bit_off(hb_to, s, o8));
        }
      }
      cnt[T_HUPS] += hup ? 1u : 0u;
      cnt[T_STEPDOWNS] += down ? 1u : 0u;
    }
    // ---- the timer rows ----
    const uint32_t tm = ee | (he << 16);
    bst32<kNT>(tm, mk_rsrc(a.timer + g0, n * 4), o4);
    if (__builtin_amdgcn_ballot_w64(redraw)) bst16<kNT>(rt, mk_rsrc(a.rt + g0, n * 2), lane * 2);
    bst8<kNT>(act, mk_rsrc(a.action + g0, n), lane);
    if (a.hb_sent) bst_mask<MT>(hb_to, opt_rsrc(static_cast<const MT *>(a.hb_sent), g0, n), lane);
    if (live) {
      cnt[T_GROUPS] += 1;
      cnt[T_CSUM] += mix64((gid * kPhi) ^ kQuorumSalt ^ (static_cast<uint64_t>(act) << 56) ^
                           (static_cast<uint64_t>(rt) << 32) ^ tm);
    }
  }
  if (a.stats) {
    const int idx[T_N] = {QE_STAT_GROUPS, QE_STAT_ELECTIONS, QE_STAT_STEPDOWNS, QE_STAT_CHECKSUM};
    wave_stats_add<T_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
