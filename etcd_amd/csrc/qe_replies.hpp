// qe_replies.hpp — qe_replies: the messages the receiver-side calls sent, as a
// dense, ordered list of records in the layout qe_inbox consumes
// (include/etcd_quorum.h states the rules).
//
// The step kernels report a receiver's send as a result code and a few rows:
// the MsgAppResp / MsgHeartbeatResp of qe_follower_step (handleAppendEntries,
// handleHeartbeat, raft/raft.go:1475-1516) and of qe_snapshot_step
// (handleSnapshot, :1518-1529), the Msg{Pre}VoteResp and the Msg{Pre}Vote
// requests of qe_vote_step (:913, :968, :977, campaign :785-835) and the
// MsgTimeoutNow of qe_progress_step (sendTimeoutNow, :1722-1724).  Everything a
// record needs is in those rows and the sender's term.
//
// The three passes of the record-list layer (qe_list.hpp): k_replies_count and
// k_replies_fill.  The counts read only bytes: the three result rows, v_req_to
// under the ballot of the lanes that campaign, and timeout_now where it is
// given.  A tile: one lane per group; the results, then the rows of each kind
// under the ballot of the lanes that need them, then the records kind by kind
// (F, S, V response, V request slot by slot, T slot by slot).
//
// The slot count and the mask width are run-time values and there is no run
// table: one object.
#pragma once
#include "qe_list.hpp"

namespace qe {

constexpr uint32_t kRpTileMax = 64 * (3 + 2 * QE_MAX_SLOTS);  // records of one tile at most
constexpr uint64_t kRepliesSalt = 0xA0761D6478BD642Full;

struct RPArgs {
  uint64_t G, goff;
  uint32_t S;
  uint32_t wide;  // the masks are 16-bit words
  uint64_t nb;    // chunks
  // qe_replies_in
  const uint64_t *term;
  const uint8_t *f_result, *f_from;
  const uint64_t *f_resp_index, *f_reject_hint, *f_resp_log_term;
  const uint32_t *f_ctx;
  const uint8_t *s_result, *s_from;
  const uint64_t *s_resp_index;
  const uint8_t *v_result, *v_type, *v_from;
  const uint64_t *v_resp_term, *v_req_log_term;
  const void *v_req_to;
  const uint64_t *last_index;  // qe_progress
  const void *timeout_now;
  // qe_replies_out
  uint64_t cap;
  uint64_t *o_group;
  uint8_t *o_to, *o_type;
  uint64_t *o_term, *o_index, *o_log_term, *o_hint;
  uint32_t *o_ctx;
  uint8_t *o_flags;
  // scratch
  const uint64_t *offsets;
  uint32_t *counts;
  uint64_t *stats;
};

// defined in qe_inst_replies.hip
int dispatch_replies_count(const RPArgs &a, hipStream_t st);
int dispatch_replies_fill(const RPArgs &a, hipStream_t st);

// Which result codes send: the codes of a kind are consecutive.
static_assert(QE_FR_LOWER_TERM_RESP == 2 && QE_FR_HEARTBEAT_RESP == 3 && QE_FR_APP_ACCEPT == 4 &&
                  QE_FR_APP_REJECT == 5 && QE_FR_APP_STALE == 6,
              "F responses are 2..6");
static_assert(QE_SR_STALE == 2 && QE_SR_NOT_MEMBER == 3 && QE_SR_FAST_FORWARD == 4 &&
                  QE_SR_RESTORED == 5,
              "S responses are 2..5");
static_assert(QE_VR_GRANT == 3 && QE_VR_REJECT == 4 && QE_VR_CAMPAIGN_PREVOTE == 8 &&
                  QE_VR_CAMPAIGN_VOTE == 9,
              "V responses are 3..4, campaigns 8..9");
__device__ __forceinline__ bool rp_f_sends(uint32_t r) { return r - 2u <= 4u; }
__device__ __forceinline__ bool rp_s_sends(uint32_t r) { return r - 2u <= 3u; }
__device__ __forceinline__ bool rp_v_responds(uint32_t r) { return r - 3u <= 1u; }
__device__ __forceinline__ bool rp_campaigns(uint32_t r) { return r - 8u <= 1u; }

// The counts of the layer: the results and timeout_now of all rounds in flight
// together, then v_req_to round by round under the ballot of the campaigns.
// `wide`: the masks are 16-bit words.
struct RepliesCounts {
  const RPArgs &a;
  bool wide;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const uint32_t sz = wide ? 2u : 1u, full = (1u << a.S) - 1u;
    const rsrc_t rf = opt_rsrc(a.f_result, base, nc), rs = opt_rsrc(a.s_result, base, nc),
                 rv = opt_rsrc(a.v_result, base, nc);
    const rsrc_t rq = list_mask_rsrc(a.v_req_to, base, nc, sz),
                 rt = list_mask_rsrc(a.timeout_now, base, nc, sz);
    uint32_t vr[kListRounds];
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) {
      const uint32_t i = list_elem(r);
      const uint32_t fr = bld8<kNT>(rf, i), sr = bld8<kNT>(rs, i);
      vr[r] = bld8<kNT>(rv, i);
      const uint32_t mt = list_ld_mask(rt, i, wide) & full;
      k[r] = (rp_f_sends(fr) ? 1u : 0u) + (rp_s_sends(sr) ? 1u : 0u) +
             (rp_v_responds(vr[r]) ? 1u : 0u) + popc(mt);
    }
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) {
      const bool camp = rp_campaigns(vr[r]);
      if (__builtin_amdgcn_ballot_w64(camp))
        k[r] += popc(list_ld_mask(rq, list_elem(r), wide, camp) & full);
    }
  }
};

// WIDE: the masks are 16-bit words.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_replies_count(RPArgs a) {
  list_count_block(a.G, a.counts, RepliesCounts{a, WIDE});
}

enum { RP_GROUPS, RP_APP, RP_HB, RP_VRESP, RP_VREQ, RP_TN, RP_BAD, RP_VIOL, RP_CSUM, RP_N };

// The output descriptors of one tile.
struct RPOut {
  rsrc_t group, to, type, term, index, lterm, hint, ctx, flags;
};

// One record per lane with `bit`, at position pos.  -> 1 where the lane has a
// record that is not a QE_RMSG_BAD (the caller counts it by type), else 0.
__device__ __forceinline__ uint32_t rp_emit(const RPOut &d, bool stats, bool bit, uint32_t pos,
                                        uint64_t gid, uint32_t to, uint32_t type, uint64_t term,
                                        uint64_t index, uint64_t lt, uint64_t hint, uint32_t ctx,
                                        uint32_t flags, uint64_t (&cnt)[RP_N]) {
  const uint32_t p1 = bit ? pos : kOOB, p4 = bit ? pos * 4 : kOOB, p8 = bit ? pos * 8 : kOOB;
  bst64<kNT>(gid, d.group, p8);
  bst8<kNT>(to, d.to, p1);
  bst8<kNT>(type, d.type, p1);
  bst64<kNT>(term, d.term, p8);
  bst64<kNT>(index, d.index, p8);
  bst64<kNT>(lt, d.lterm, p8);
  bst64<kNT>(hint, d.hint, p8);
  bst32<kNT>(ctx, d.ctx, p4);
  bst8<kNT>(flags, d.flags, p1);
  if (stats) {
    uint64_t h = mix64((gid * kPhi) ^ kRepliesSalt ^ (static_cast<uint64_t>(type) << 56) ^
                       (static_cast<uint64_t>(to) << 48));
    h = mix64(h ^ term);
    h = mix64(h ^ index);
    h = mix64(h ^ lt);
    h = mix64(h ^ hint);
    h = mix64(h ^ (ctx | (static_cast<uint64_t>(flags) << 32)));
    const bool bad = bit && type == QE_RMSG_BAD;
    cnt[RP_BAD] += bad ? 1u : 0u;
    cnt[RP_VIOL] += bad ? 1u : 0u;
    cnt[RP_CSUM] += bit ? h : 0u;
  }
  return (stats && bit && type != QE_RMSG_BAD) ? 1u : 0u;
}

// Tile t, whose first record has position tb.
template <bool WIDE>
__device__ __forceinline__ void replies_tile(const RPArgs &a, uint64_t t, uint64_t tb,
                                             uint32_t lane, uint64_t (&cnt)[RP_N]) {
  constexpr bool wide = WIDE;
  const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
  const bool stats = a.stats != nullptr;
  const uint32_t sz = wide ? 2u : 1u, S = a.S, full = (1u << S) - 1u;
  // ---- 1. the results and the masks: who sends what (a lane past n reads 0) ----
  const uint32_t fr = bld8<kNT>(opt_rsrc(a.f_result, g0, n), lane);
  const uint32_t sr = bld8<kNT>(opt_rsrc(a.s_result, g0, n), lane);
  const uint32_t vr = bld8<kNT>(opt_rsrc(a.v_result, g0, n), lane);
  const uint32_t mt = list_ld_mask(list_mask_rsrc(a.timeout_now, g0, n, sz), lane, wide) & full;
  const bool is_f = rp_f_sends(fr), is_s = rp_s_sends(sr), is_v = rp_v_responds(vr),
             camp = rp_campaigns(vr);
  uint32_t mq = 0;
  if (__builtin_amdgcn_ballot_w64(camp))
    mq = list_ld_mask(list_mask_rsrc(a.v_req_to, g0, n, sz), lane, wide, camp) & full;
  // ---- 2. the rows of each kind, under the ballot of the lanes that need them ----
  const bool need_t = is_f || is_s || mt != 0;
  uint64_t term = 0;
  if (__builtin_amdgcn_ballot_w64(need_t))
    term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), need_t ? o8 : kOOB);
  uint32_t f_to = 0, f_ctx = 0;
  uint64_t f_idx = 0, f_hint = 0, f_lt = 0;
  const bool f_rej = fr == QE_FR_APP_REJECT, f_hb = fr == QE_FR_HEARTBEAT_RESP;
  if (__builtin_amdgcn_ballot_w64(is_f)) {
    f_to = bld8<kNT>(mk_rsrc(a.f_from + g0, n), is_f ? lane : kOOB);
    const bool wi = fr >= QE_FR_APP_ACCEPT && is_f;  // accept, reject, stale
    f_idx = bld64<kNT>(mk_rsrc(a.f_resp_index + g0, n * 8), wi ? o8 : kOOB);
    if (__builtin_amdgcn_ballot_w64(f_rej)) {
      f_hint = bld64<kNT>(mk_rsrc(a.f_reject_hint + g0, n * 8), f_rej ? o8 : kOOB);
      f_lt = bld64<kNT>(mk_rsrc(a.f_resp_log_term + g0, n * 8), f_rej ? o8 : kOOB);
    }
    if (__builtin_amdgcn_ballot_w64(f_hb))
      f_ctx = bld32<kNT>(opt_rsrc(a.f_ctx, g0, n), f_hb ? lane * 4 : kOOB);
  }
  uint32_t s_to = 0;
  uint64_t s_idx = 0;
  if (__builtin_amdgcn_ballot_w64(is_s)) {
    s_to = bld8<kNT>(mk_rsrc(a.s_from + g0, n), is_s ? lane : kOOB);
    s_idx = bld64<kNT>(mk_rsrc(a.s_resp_index + g0, n * 8), is_s ? o8 : kOOB);
  }
  uint32_t v_to = 0, v_ty = 0;
  uint64_t v_term = 0, v_lt = 0, v_li = 0;
  if (__builtin_amdgcn_ballot_w64(is_v || camp)) {
    const bool need_ty = is_v || vr == QE_VR_CAMPAIGN_VOTE;  // the response's type, or FORCE
    v_ty = bld8<kNT>(mk_rsrc(a.v_type + g0, n), need_ty ? lane : kOOB);
    v_term = bld64<kNT>(mk_rsrc(a.v_resp_term + g0, n * 8), (is_v || camp) ? o8 : kOOB);
    if (__builtin_amdgcn_ballot_w64(is_v))
      v_to = bld8<kNT>(mk_rsrc(a.v_from + g0, n), is_v ? lane : kOOB);
    if (__builtin_amdgcn_ballot_w64(camp)) {
      v_lt = bld64<kNT>(mk_rsrc(a.v_req_log_term + g0, n * 8), camp ? o8 : kOOB);
      v_li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), camp ? o8 : kOOB);
    }
  }
  // ---- 3. the records, kind by kind ----
  // what of the arrays this tile may write: capacity is the descriptors'
  const auto [tbc, rem] = list_room(tb, a.cap, kRpTileMax);
  const RPOut d = {mk_rsrc(a.o_group + tbc, rem * 8),
                   mk_rsrc(a.o_to + tbc, rem),
                   mk_rsrc(a.o_type + tbc, rem),
                   mk_rsrc(a.o_term + tbc, rem * 8),
                   mk_rsrc(a.o_index + tbc, rem * 8),
                   mk_rsrc(a.o_log_term + tbc, rem * 8),
                   mk_rsrc(a.o_hint + tbc, rem * 8),
                   a.o_ctx ? mk_rsrc(a.o_ctx + tbc, rem * 4) : mk_rsrc(a.o_ctx, 0),
                   a.o_flags ? mk_rsrc(a.o_flags + tbc, rem) : mk_rsrc(a.o_flags, 0)};
  uint32_t pbase = 0;
  // F: MsgAppResp / MsgHeartbeatResp of qe_follower_step
  uint64_t bal = __builtin_amdgcn_ballot_w64(is_f);
  if (bal) {
    const bool ok = f_to < S;
    const uint32_t type = !ok     ? QE_RMSG_BAD
                          : f_hb  ? QE_IMSG_HEARTBEAT_RESP
                          : f_rej ? QE_IMSG_APP_RESP_REJECT
                                  : QE_IMSG_APP_RESP;
    const bool c = rp_emit(d, stats, is_f, pbase + lane_rank(bal), gid, f_to, type, term,
                           ok ? f_idx : 0, ok ? f_lt : 0, ok ? f_hint : 0, ok ? f_ctx : 0u, 0u, cnt);
    cnt[RP_HB] += (c && f_hb) ? 1u : 0u;
    cnt[RP_APP] += (c && !f_hb) ? 1u : 0u;
    pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
  }
  // S: MsgAppResp of qe_snapshot_step
  bal = __builtin_amdgcn_ballot_w64(is_s);
  if (bal) {
    const bool ok = s_to < S;
    cnt[RP_APP] += rp_emit(d, stats, is_s, pbase + lane_rank(bal), gid, s_to,
                           ok ? QE_IMSG_APP_RESP : QE_RMSG_BAD, term, ok ? s_idx : 0, 0, 0, 0u, 0u,
                           cnt);
    pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
  }
  // V response: Msg{Pre}VoteResp
  bal = __builtin_amdgcn_ballot_w64(is_v);
  if (bal) {
    const uint32_t ty = v_ty == QE_VMSG_VOTE      ? QE_IMSG_VOTE_RESP
                        : v_ty == QE_VMSG_PREVOTE ? QE_IMSG_PREVOTE_RESP
                                                  : QE_RMSG_BAD;
    const uint32_t type = v_to < S ? ty : QE_RMSG_BAD;
    const uint32_t fl = (type != QE_RMSG_BAD && vr == QE_VR_REJECT) ? QE_VMF_REJECT : 0u;
    cnt[RP_VRESP] += rp_emit(d, stats, is_v, pbase + lane_rank(bal), gid, v_to, type, v_term, 0,
                             0, 0, 0u, fl, cnt);
    pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
  }
  // V request: Msg{Pre}Vote to every slot of req_to
  const uint32_t uq = wave_or(mq);
  if (uq) {
    const uint32_t type = vr == QE_VR_CAMPAIGN_VOTE ? QE_IMSG_VOTE : QE_IMSG_PREVOTE;
    const uint32_t fl =
        (vr == QE_VR_CAMPAIGN_VOTE && v_ty == QE_VMSG_TIMEOUT_NOW) ? QE_VMF_FORCE : 0u;
    for (uint32_t s = 0; s < S; s++) {
      if (!((uq >> s) & 1u)) continue;
      const bool bit = (mq >> s) & 1u;
      bal = __builtin_amdgcn_ballot_w64(bit);
      cnt[RP_VREQ] += rp_emit(d, stats, bit, pbase + lane_rank(bal), gid, s, type, v_term, v_li,
                              v_lt, 0, 0u, fl, cnt);
      pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
    }
  }
  // T: MsgTimeoutNow to every slot of timeout_now
  const uint32_t ut = wave_or(mt);
  if (ut) {
    for (uint32_t s = 0; s < S; s++) {
      if (!((ut >> s) & 1u)) continue;
      const bool bit = (mt >> s) & 1u;
      bal = __builtin_amdgcn_ballot_w64(bit);
      cnt[RP_TN] += rp_emit(d, stats, bit, pbase + lane_rank(bal), gid, s, QE_IMSG_TIMEOUT_NOW,
                            term, 0, 0, 0, 0u, 0u, cnt);
      pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
    }
  }
  cnt[RP_GROUPS] += (is_f || is_s || is_v || mq != 0 || mt != 0) ? 1u : 0u;
}

// WIDE as k_replies_count's.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_replies_fill(RPArgs a) {
  const int idx[RP_N] = {QE_STAT_GROUPS,          QE_STAT_REPLY_APP_RESP,
                         QE_STAT_REPLY_HEARTBEAT_RESP, QE_STAT_REPLY_VOTE_RESP,
                         QE_STAT_REPLY_VOTE_REQ,  QE_STAT_REPLY_TIMEOUT_NOW,
                         QE_STAT_REPLY_BAD,       QE_STAT_INVARIANT_VIOLATIONS,
                         QE_STAT_CHECKSUM};
  list_fill_walk<replies_tile<WIDE>>(a, idx, RepliesCounts{a, WIDE});
}

}  // namespace qe
