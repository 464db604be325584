// qe_requests.hpp — qe_requests: a list of client requests (MsgProp,
// MsgReadIndex, MsgTransferLeader) and MsgReadIndexResp handled as raft.Step
// would on their receiver: routed into the leader-side rows, forwarded,
// answered or dropped by role (include/etcd_quorum.h states the rules;
// tests/requests_model.py restates them sequentially).
//
// The sequential rule (per group, walk the records in list order until the
// first one that writes a row, which closes the group; every later record of
// the group is deferred) has an exact order-free form.  The key of record i is
// i + 1.  One scratch word per group (qe_route.hpp: all-ones = none, the result
// of 32-bit atomicMin, so any arrival order gives the same bit-exact outputs):
//   stop[g]   lowest key of a closer of g: at a leader a valid PROP /
//             READ_INDEX / TRANSFER_LEADER whose term is 0 or r.Term, in any
//             state a valid record with term > r.Term.
// A record is deferred iff key > stop[g], the closer iff key == stop[g], and
// stateless otherwise: whether a record is a closer depends on the record and
// the resident rows alone, never on another record.
//
// Kernels, ordered by kernel boundaries alone (no spin wait, no look-back):
//   k_requests_init   G-sized: stop and the complete rows;
//   k_requests_stop   stop (reads f->term, f->state);
//   k_requests_route  dispositions, the scatter into the rows, two flag bytes
//                     per record (deferred; the kind of its output record),
//                     the statistics;
//   k_collect_count / k_collect_scan (qe_collect.hpp) over each of the two flag
//   arrays, then the fill of the record-list layer (qe_list.hpp) with a record
//   as the layer's element: k_requests_out writes the output records, the
//   routing layer's k_route_positions the positions of the deferred ones.
// The lanes, the tiles and the addressing are the routing layer's.
#pragma once
#include "qe_route.hpp"

namespace qe {

constexpr uint64_t kRequestsSalt = 0xA24BAED4963EE407ull;

struct RQArgs {
  uint64_t G, goff, stride, n, cc_stride;
  uint32_t S, max_cc, flags;
  // qe_follower
  const uint64_t *fterm;
  const uint8_t *fstate, *flead;
  // qe_requests_in
  const uint64_t *group;
  const uint8_t *type, *from;
  const uint64_t *term, *key;
  const uint32_t *num_entries;
  const uint64_t *payload;
  const uint8_t *cc_count;
  const uint32_t *cc_pos;
  const uint8_t *cc_leave;
  const uint32_t *cc_size;
  // qe_requests_out: the rows
  uint32_t *p_num_entries;
  uint64_t *p_payload;
  uint8_t *p_cc_count;
  uint32_t *p_cc_pos;
  uint8_t *p_cc_leave;
  uint32_t *p_cc_size;
  uint8_t *ri_request;
  uint64_t *ri_key;
  uint8_t *ri_from;
  uint8_t *v_type, *v_from;
  uint64_t *v_term, *v_index, *v_log_term;
  uint8_t *v_flags;
  uint8_t *r_type;
  uint32_t *p_src, *ri_src, *v_src, *r_src;
  uint8_t *disposition;
  // scratch
  uint32_t *stop;        // [G]
  uint8_t *dflag, *okind;  // [n] 1 = deferred; QE_QO_* of the record's output record, 0 = none
  uint64_t *stats;
};

// The arguments of the output list's fill: the layer's element is a record, so
// its G is the list's length.
struct RQList {
  uint64_t G, nb, goff;
  const uint64_t *offsets;
  uint64_t *stats;  // NULL: the routing pass holds the statistics
  const uint8_t *flag;  // [n] okind
  // qe_follower, qe_progress
  const uint64_t *fterm;
  const uint8_t *flead, *self_slot;
  uint32_t S;
  // qe_requests_in
  const uint64_t *group;
  const uint8_t *type, *from;
  const uint64_t *index, *key;
  // qe_requests_out: the list
  uint64_t cap;
  uint64_t *o_group;
  uint8_t *o_kind, *o_type, *o_to, *o_from;
  uint64_t *o_term, *o_index, *o_key;
  uint32_t *o_src;
};

// defined in qe_inst_route.hip
int dispatch_requests_init(const RQArgs &a, hipStream_t st);
int dispatch_requests_passes(const RQArgs &a, hipStream_t st);
int dispatch_requests_out(const RQList &a, hipStream_t st);

#ifdef QE_ROUTE_KERNELS

// Record `lane` of tile t: its head, its term and whether it takes part (rule 1).
struct QRec : RouteRec {
  uint64_t term;
  bool valid;
};
__device__ __forceinline__ QRec requests_rec(const RQArgs &a, uint64_t t, uint32_t lane) {
  const uint32_t cnt = tile_n(a.n, t);
  QRec r;
  route_rec(r, a.group, a.from, a.type, a.n, a.goff, t, lane);
  r.term = bld64<kNT>(mk_rsrc(a.term + t * 64, cnt * 8), lane * 8);
  const uint32_t ne = bld32<kNT>(opt_rsrc(a.num_entries, t * 64, cnt),
                                 r.type == QE_QMSG_PROP ? lane * 4 : kOOB);
  const bool known = r.type == QE_QMSG_TRANSFER_LEADER ||
                     (r.type >= QE_QMSG_PROP && r.type <= QE_QMSG_READ_INDEX_RESP);
  const bool local = r.type == QE_QMSG_PROP || r.type == QE_QMSG_READ_INDEX;
  r.valid = r.live && r.g < a.G && known && (r.from < a.S || r.from == 0xFFu) &&
            !(r.type == QE_QMSG_PROP && ne == 0) && !(local && r.term != 0) &&
            !(r.type == QE_QMSG_TRANSFER_LEADER && r.from == 0xFFu);
  return r;
}

// Whether a valid record closes its group (rule 4): it writes a row.
__device__ __forceinline__ bool requests_closer(const QRec &r, uint64_t rterm, uint32_t state) {
  if (r.term != 0 && r.term > rterm) return true;
  return state == QE_STATE_LEADER && r.type != QE_QMSG_READ_INDEX_RESP &&
         (r.term == 0 || r.term == rterm);
}

// The init pass, one thread per group: the scratch word and the complete rows.
__global__ __launch_bounds__(kBlock) void k_requests_init(RQArgs a) {
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g < a.G;
       g += static_cast<uint64_t>(gridDim.x) * kBlock) {
    a.stop[g] = kRouteNone;
    a.p_num_entries[g] = 0;
    a.ri_request[g] = 0;
    a.v_type[g] = QE_VMSG_NONE;
    for (uint32_t s = 0; s < a.S; s++) a.r_type[s * a.stride + g] = QE_MSG_NONE;
  }
}

// The key pass: stop.
__global__ __launch_bounds__(kBlock) void k_requests_stop(RQArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.n, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const QRec r = requests_rec(a, t, lane);
    if (r.valid && requests_closer(r, a.fterm[r.g], a.fstate[r.g])) atomicMin(a.stop + r.g, r.key);
  }
}

enum {
  RQ_GROUPS, RQ_ROUTED, RQ_STEPDOWN, RQ_DEFERRED, RQ_LOWER, RQ_NO_ARM, RQ_FORWARDED, RQ_READ_STATE,
  RQ_PROP_DROPPED, RQ_NO_LEADER, RQ_REF_PANIC, RQ_BAD, RQ_VIOL, RQ_CSUM, RQ_N
};

// The routing pass: the dispositions, the rows, the two flag bytes.
__global__ __launch_bounds__(kBlock) void k_requests_route(RQArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.n, lane, wave, nwaves, ntiles);
  uint64_t cnt[RQ_N] = {};
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const QRec r = requests_rec(a, t, lane);
    const uint64_t r0 = t * 64;
    const uint32_t n = tile_n(a.n, t);
    const uint32_t pos = r.key - 1u;
    // ---- the receiver's rows, the disposition (rules 2-4) ----
    uint32_t stop = kRouteNone, state = 0, lead = 0xFFu;
    uint64_t rterm = 0;
    if (r.valid) {
      stop = a.stop[r.g];
      rterm = a.fterm[r.g];
      state = a.fstate[r.g];
      lead = a.flead[r.g];
    }
    const bool has_lead = lead < a.S;
    const bool prop = r.type == QE_QMSG_PROP, ri = r.type == QE_QMSG_READ_INDEX;
    const bool tl = r.type == QE_QMSG_TRANSFER_LEADER, resp = r.type == QE_QMSG_READ_INDEX_RESP;
    uint32_t disp = QE_QD_BAD, kind = 0;
    if (r.valid) {
      if (r.key > stop) {
        disp = QE_QD_DEFERRED;
      } else if (r.term != 0 && r.term < rterm) {
        disp = QE_QD_DROP_LOWER_TERM;
      } else if (r.term != 0 && r.term > rterm) {  // (the closer: key == stop)
        disp = QE_QD_STEPDOWN;
        kind = resp ? QE_QO_READ_STATE : 0u;
      } else if (state == QE_STATE_LEADER) {
        disp = resp ? QE_QD_NO_ARM : QE_QD_ROUTED;
      } else if (state == QE_STATE_CANDIDATE || state == QE_STATE_PRE_CANDIDATE) {
        disp = prop ? QE_QD_PROP_DROPPED : QE_QD_NO_ARM;
        kind = prop ? QE_QO_PROP_DROPPED : 0u;
      } else if (resp) {
        disp = QE_QD_READ_STATE;
        kind = QE_QO_READ_STATE;
      } else if (prop) {
        const bool fwd = has_lead && !(a.flags & QE_REQ_NO_FORWARD);
        disp = fwd ? QE_QD_FORWARDED : QE_QD_PROP_DROPPED;
        kind = fwd ? QE_QO_FWD : QE_QO_PROP_DROPPED;
      } else if (!has_lead) {
        disp = QE_QD_NO_LEADER;
      } else if (tl && r.term != 0) {
        disp = QE_QD_REF_PANIC;
      } else {
        disp = QE_QD_FORWARDED;
        kind = QE_QO_FWD;
      }
    }
    const bool routed = disp == QE_QD_ROUTED, down = disp == QE_QD_STEPDOWN;
    // ---- the fields of the records that go into a row ----
    const bool rp = routed && prop, rr = routed && ri, rt = routed && tl;
    const uint32_t ne = bld32<kNT>(opt_rsrc(a.num_entries, r0, n), rp ? lane * 4 : kOOB);
    const uint64_t payload = bld64<kNT>(opt_rsrc(a.payload, r0, n), rp ? lane * 8 : kOOB);
    const uint32_t ccn = bld8<kNT>(opt_rsrc(a.cc_count, r0, n), rp ? lane : kOOB);
    const uint64_t key = bld64<kNT>(mk_rsrc(a.key + r0, n * 8), rr ? lane * 8 : kOOB);
    // ---- the stores ----
    bst8<kNT>(disp, mk_rsrc(a.disposition + r0, n), lane);
    bst8<kNT>(disp == QE_QD_DEFERRED ? 1u : 0u, mk_rsrc(a.dflag + r0, n), lane);
    bst8<kNT>(kind, mk_rsrc(a.okind + r0, n), lane);
    const uint64_t g = r.g;
    if (rp) {
      a.p_num_entries[g] = ne;
      if (a.p_payload) a.p_payload[g] = payload;
      if (a.p_cc_count) a.p_cc_count[g] = static_cast<uint8_t>(ccn);
      if (a.p_src) a.p_src[g] = pos;
    }
    // the conf-change rows of a routed proposal: every one of the max_cc rows,
    // zeros included (a wave without one issues nothing)
    if (a.max_cc && __builtin_amdgcn_ballot_w64(rp)) {
      for (uint32_t k = 0; k < a.max_cc; k++) {
        const uint64_t row = static_cast<uint64_t>(k) * a.n + r0;
        const uint32_t cp = bld32<kNT>(opt_rsrc(a.cc_pos, row, n), rp ? lane * 4 : kOOB);
        const uint32_t cl = bld8<kNT>(opt_rsrc(a.cc_leave, row, n), rp ? lane : kOOB);
        const uint32_t cs = bld32<kNT>(opt_rsrc(a.cc_size, row, n), rp ? lane * 4 : kOOB);
        if (rp) {
          a.p_cc_pos[k * a.cc_stride + g] = cp;
          a.p_cc_leave[k * a.cc_stride + g] = static_cast<uint8_t>(cl);
          a.p_cc_size[k * a.cc_stride + g] = cs;
        }
      }
    }
    if (rr) {
      a.ri_request[g] = 1;
      a.ri_key[g] = key;
      a.ri_from[g] = static_cast<uint8_t>(r.from);
      if (a.ri_src) a.ri_src[g] = pos;
    }
    if (rt) {
      const uint64_t k = r.from * a.stride + g;
      a.r_type[k] = QE_MSG_TRANSFER_LEADER;
      if (a.r_src) a.r_src[k] = pos;
    }
    if (down) {
      a.v_type[g] = QE_VMSG_VOTE_RESP;
      a.v_from[g] = static_cast<uint8_t>(r.from);
      a.v_term[g] = r.term;
      a.v_index[g] = 0;
      a.v_log_term[g] = 0;
      if (a.v_flags) a.v_flags[g] = QE_VMF_REJECT;
      if (a.v_src) a.v_src[g] = pos;
    }
    if (a.stats) {
      const bool bad = r.live && !r.valid, panic = disp == QE_QD_REF_PANIC;
      cnt[RQ_GROUPS] += routed ? 1u : 0u;  // (a group has one ROUTED record at most)
      cnt[RQ_ROUTED] += routed ? 1u : 0u;
      cnt[RQ_STEPDOWN] += down ? 1u : 0u;
      cnt[RQ_DEFERRED] += disp == QE_QD_DEFERRED ? 1u : 0u;
      cnt[RQ_LOWER] += disp == QE_QD_DROP_LOWER_TERM ? 1u : 0u;
      cnt[RQ_NO_ARM] += disp == QE_QD_NO_ARM ? 1u : 0u;
      cnt[RQ_FORWARDED] += disp == QE_QD_FORWARDED ? 1u : 0u;
      cnt[RQ_READ_STATE] += disp == QE_QD_READ_STATE ? 1u : 0u;
      cnt[RQ_PROP_DROPPED] += disp == QE_QD_PROP_DROPPED ? 1u : 0u;
      cnt[RQ_NO_LEADER] += disp == QE_QD_NO_LEADER ? 1u : 0u;
      cnt[RQ_REF_PANIC] += panic ? 1u : 0u;
      cnt[RQ_BAD] += bad ? 1u : 0u;
      cnt[RQ_VIOL] += (bad || panic) ? 1u : 0u;
      cnt[RQ_CSUM] += r.live ? route_hash(r.gid, kRequestsSalt, disp, r.type, r.from, pos) : 0u;
    }
  }
  if (a.stats) {
    const int idx[RQ_N] = {QE_STAT_GROUPS,          QE_STAT_REQ_ROUTED,       QE_STAT_REQ_STEPDOWN,
                          QE_STAT_REQ_DEFERRED,    QE_STAT_REQ_LOWER_TERM,   QE_STAT_REQ_NO_ARM,
                          QE_STAT_REQ_FORWARDED,   QE_STAT_REQ_READ_STATE,   QE_STAT_REQ_PROP_DROPPED,
                          QE_STAT_REQ_NO_LEADER,   QE_STAT_REQ_REF_PANIC,    QE_STAT_REQ_BAD,
                          QE_STAT_INVARIANT_VIOLATIONS, QE_STAT_CHECKSUM};
    wave_stats_add<RQ_N>(cnt, idx, a.stats);
  }
}

// Tile t of the list, whose first output record has position tb (rule 5).
__device__ __forceinline__ void requests_out_tile(const RQList &a, uint64_t t, uint64_t tb,
                                                  uint32_t lane, uint64_t (&)[1]) {
  const uint64_t r0 = t * 64;
  const uint32_t n = tile_n(a.G, t);
  // ---- 1. who has a record, and of what kind ----
  const uint32_t kind = bld8<kNT>(mk_rsrc(a.flag + r0, n), lane);
  const bool has = kind != 0, fwd = kind == QE_QO_FWD;
  const uint32_t h1 = has ? lane : kOOB, h8 = has ? lane * 8 : kOOB;
  // ---- 2. the record's fields, the receiver's rows (a record with a kind is
  //         valid: its group is in the batch) ----
  const uint64_t gid = bld64<kNT>(mk_rsrc(a.group + r0, n * 8), h8);
  const uint32_t type = bld8<kNT>(mk_rsrc(a.type + r0, n), h1);
  const uint32_t from = bld8<kNT>(mk_rsrc(a.from + r0, n), h1);
  const uint64_t index = bld64<kNT>(mk_rsrc(a.index + r0, n * 8),
                                    kind == QE_QO_READ_STATE ? lane * 8 : kOOB);
  const uint64_t key = bld64<kNT>(mk_rsrc(a.key + r0, n * 8), h8);
  uint32_t to = 0xFFu, ofrom = 0xFFu;
  uint64_t term = 0;
  if (fwd) {
    const uint64_t g = gid - a.goff;
    to = a.flead[g];
    ofrom = from < a.S ? from : a.self_slot[g];
    if (type == QE_QMSG_TRANSFER_LEADER) term = a.fterm[g];
  }
  // ---- 3. the stores: the records of the tile in lane order ----
  const uint64_t bal = __builtin_amdgcn_ballot_w64(has);
  const uint32_t pos = lane_rank(bal);
  const auto [tbc, rem] = list_room(tb, a.cap, 64);
  const uint32_t p1 = has ? pos : kOOB, p4 = has ? pos * 4 : kOOB, p8 = has ? pos * 8 : kOOB;
  bst64<kNT>(gid, mk_rsrc(a.o_group + tbc, rem * 8), p8);
  bst8<kNT>(kind, mk_rsrc(a.o_kind + tbc, rem), p1);
  bst8<kNT>(type, mk_rsrc(a.o_type + tbc, rem), p1);
  bst8<kNT>(to, mk_rsrc(a.o_to + tbc, rem), p1);
  bst8<kNT>(ofrom, mk_rsrc(a.o_from + tbc, rem), p1);
  bst64<kNT>(term, mk_rsrc(a.o_term + tbc, rem * 8), p8);
  bst64<kNT>(index, mk_rsrc(a.o_index + tbc, rem * 8), p8);
  bst64<kNT>(key, mk_rsrc(a.o_key + tbc, rem * 8), p8);
  bst32<kNT>(static_cast<uint32_t>(r0) + lane, mk_rsrc(a.o_src + tbc, rem * 4), p4);
}

__global__ __launch_bounds__(kBlock) void k_requests_out(RQList a) {
  const int idx[1] = {QE_STAT_GROUPS};
  list_fill_walk<requests_out_tile>(a, idx, FlagCounts{a.flag});
}
#endif  // QE_ROUTE_KERNELS

}  // namespace qe
