// qe_applyconf.hpp — qe_apply_conf: a list of committed conf-change entries
// applied as RawNode.ApplyConfChange does (raft/raft.go:1623-1700), on every
// role: the decode of the ConfChangeV2 (raft/raftpb/confchange.go:71-107), the
// Changer of qe_conf.hpp on the group's resident configuration, initProgress
// for the created slots, and for a leader the `switched` byte the switch
// kernel (k_switch_config) then runs on (include/etcd_quorum.h states the
// rules; tests/apply_conf_model.py restates them sequentially).
//
// The list is in non-decreasing group order, so the records of one group are
// a run of neighbours.  A record whose predecessor has another group is the
// run's head; the head's thread walks the run in list order with the group's
// configuration in registers, so two records of one group never race and no
// atomic is needed.  Every other thread leaves at once.
//
// Kernels, ordered by kernel boundaries alone:
//   k_apply_conf_clear   the `switched` row of the scratch, 16 B per store;
//   k_apply_conf<S>      the heads: decode, Changer, the rows of c and p, the
//                        per-record results and ConfStates, switched[g] = 1
//                        for a leader's applied record;
//   k_switch_config      (qe_progress.hpp, through its own dispatch) on the
//                        switched row;
//   k_apply_conf_gather  sw_result of the QE_AC_LEADER records from the switch
//                        kernel's result row.
// A record's fields sit in record-major rows, read through the tile's buffer
// descriptor where the tile's lanes read them (the head test) and by plain
// loads on the head's walk, whose records may lie in any later tile; a group's
// rows are reached by plain loads and stores under the head's branch, as
// k_requests_route reaches them.
#pragma once
#include "qe_conf.hpp"

namespace qe {

int hip_status(hipError_t e);

struct ACArgs {
  uint64_t G, goff, pstride;
  uint64_t cap, n;        // the list's capacity; the records when count is NULL
  const uint64_t *count;  // device, or NULL
  uint32_t C;
  // qe_conf
  uint64_t *ids;
  void *inc, *out, *lrn, *lnx, *isl, *trk;
  uint8_t *auto_leave;
  // qe_progress: the mask rows that are other memory than c's (else NULL), the
  // Progress rows, lastIndex; qe_follower: the role
  void *p_inc, *p_out, *p_trk;
  uint64_t *p_match, *p_next, *p_pending;
  uint32_t *p_pw;
  const uint64_t *last_index;
  const uint8_t *fstate;
  // qe_apply_conf_in
  const uint64_t *group;
  const uint8_t *transition, *nchanges;
  const uint8_t *type;   // [C][cap]
  const uint64_t *node;  // [C][cap]
  const uint8_t *slot;   // [C][cap] or NULL
  // qe_apply_conf_out
  uint8_t *result, *cc_result, *sw_result;
  void *o_inc, *o_out, *o_lrn, *o_lnx, *o_trk, *o_newp;
  uint8_t *o_al;
  uint64_t *o_ids;  // [S][cap] or NULL
  // scratch
  uint8_t *switched;     // [G]
  const uint8_t *swres;  // [G] the switch kernel's result row
};

// defined in qe_inst_applyconf.hip
int dispatch_apply_conf_clear(uint8_t *row, uint64_t bytes, hipStream_t st);
int dispatch_apply_conf(const ACArgs &a, uint32_t S, hipStream_t st);
int dispatch_apply_conf_gather(const ACArgs &a, hipStream_t st);

#ifdef QE_APPLYCONF_KERNELS

// The records of the call: the device count clamped to the capacity, or n.
__device__ __forceinline__ uint64_t ac_records(const ACArgs &a) {
  if (!a.count) return a.n;
  const uint64_t c = *a.count;
  return c < a.cap ? c : a.cap;
}

template <typename MT>
__device__ __forceinline__ uint32_t ac_ld(const void *row, uint64_t k) {
  return static_cast<const MT *>(row)[k];
}
template <typename MT>
__device__ __forceinline__ void ac_st(void *row, uint64_t k, uint32_t v) {
  static_cast<MT *>(row)[k] = static_cast<MT>(v);
}

// Record j's outputs: the three result bytes (sw_result is the gather's) and
// the ConfState after the record.
template <int S, typename MT>
__device__ __forceinline__ void ac_out(const ACArgs &a, uint64_t j, uint32_t res, uint32_t ccr,
                                       const CCState &c, const uint64_t (&id)[kCCMax],
                                       uint32_t created) {
  a.result[j] = static_cast<uint8_t>(res);
  a.cc_result[j] = static_cast<uint8_t>(ccr);
  a.sw_result[j] = QE_SW_NONE;
  ac_st<MT>(a.o_inc, j, c.inc);
  ac_st<MT>(a.o_out, j, c.out);
  ac_st<MT>(a.o_lrn, j, c.lrn);
  ac_st<MT>(a.o_lnx, j, c.lnx);
  ac_st<MT>(a.o_trk, j, c.trk);
  ac_st<MT>(a.o_newp, j, created);
  a.o_al[j] = static_cast<uint8_t>(c.al);
  if (a.o_ids) {
#pragma unroll
    for (int s = 0; s < S; s++) a.o_ids[static_cast<uint64_t>(s) * a.cap + j] = ((c.trk >> s) & 1u) ? id[s] : 0ull;
  }
}

// The run of records [i, ...) of group gid, walked by its head's thread.
template <int S, typename MT>
__device__ __forceinline__ void ac_run(const ACArgs &a, uint64_t n, uint64_t i, uint64_t gid,
                                       bool bad_order) {
  constexpr uint32_t full = (1u << S) - 1u;
  const uint64_t g = gid - a.goff;
  uint64_t id[kCCMax];
#pragma unroll
  for (int s = 0; s < kCCMax; s++) id[s] = 0;
  // ---- a run with no group to work on: its head's code, then SKIPPED ----
  if (bad_order || g >= a.G) {
    const CCState none{0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t j = i; j < n && (j == i || a.group[j] == gid); j++)
      ac_out<S, MT>(a, j, j != i ? QE_AC_SKIPPED : (bad_order ? QE_AC_BAD_ORDER : QE_AC_BAD_GROUP),
                    QE_CC_OK, none, id, 0u);
    return;
  }
  // ---- the group's configuration as qe_confchange reads it: the words as
  //      they lie in memory (what a store is compared with), the masks cut to
  //      S slots, the IDs of the tracked slots ----
  uint32_t m_inc = ac_ld<MT>(a.inc, g), m_out = ac_ld<MT>(a.out, g), m_lrn = ac_ld<MT>(a.lrn, g),
           m_lnx = ac_ld<MT>(a.lnx, g), m_isl = ac_ld<MT>(a.isl, g), m_trk = ac_ld<MT>(a.trk, g);
  CCState c{m_inc & full, m_out & full, m_lrn & full, m_lnx & full, m_isl & full, m_trk & full,
            a.auto_leave[g] != 0 ? 1u : 0u, 0u};
#pragma unroll
  for (int s = 0; s < S; s++)
    if ((c.trk >> s) & 1u) id[s] = a.ids[static_cast<uint64_t>(s) * a.G + g];
  const uint64_t li = a.last_index[g];
  const bool leader = a.fstate[g] == QE_STATE_LEADER;
  bool refused = false, led = false;
  for (uint64_t j = i; j < n && (j == i || a.group[j] == gid); j++) {
    uint32_t res, ccr = QE_CC_OK, created = 0;
    if (refused) {
      res = QE_AC_SKIPPED;
    } else if (led) {
      res = QE_AC_DEFERRED;
    } else {
      const uint32_t tr = a.transition[j], cnt = a.nchanges[j];
      if (tr > QE_AC_JOINT_EXPLICIT || cnt > a.C) {
        res = QE_AC_BAD_CHANGE;
      } else {
        // ConfChangeV2.LeaveJoint / EnterJoint (confchange.go:71-107)
        const uint32_t op = (cnt == 0 && tr == QE_AC_AUTO) ? QE_CC_OP_LEAVE_JOINT
                            : (tr != QE_AC_AUTO || cnt > 1)
                                ? (tr != QE_AC_JOINT_EXPLICIT ? QE_CC_OP_ENTER_JOINT_AUTO
                                                              : QE_CC_OP_ENTER_JOINT)
                                : QE_CC_OP_SIMPLE;
        CCState c2 = c;
        c2.newp = 0;
        uint64_t id2[kCCMax];
#pragma unroll
        for (int s = 0; s < kCCMax; s++) id2[s] = id[s];
        const int rc = cc_change<S>(op, c2, id2, [&](CCState &cs, uint64_t (&ids)[kCCMax]) -> int {
          for (uint32_t k = 0; k < cnt; k++) {
            const uint64_t e = static_cast<uint64_t>(k) * a.cap + j;
            const int r1 = cc_one<S, true>(cs, ids, a.node[e], a.type[e], a.slot ? a.slot[e] : kCCAnySlot);
            if (r1) return r1;
          }
          return cs.inc == 0 ? QE_CC_ERR_REMOVED_ALL : QE_CC_OK;
        });
        if (rc != QE_CC_OK) {  // the reference's panic (:1637-1640): the state stays
          res = QE_AC_CHANGER_ERROR;
          ccr = static_cast<uint32_t>(rc);
        } else {
          res = leader ? QE_AC_LEADER : QE_AC_APPLIED;
          led = leader;
          created = c2.newp & c2.trk;
          c2.isl &= c2.trk;
          // the rows of c: only the words the change rewrote (cc_finish)
          if (c2.inc != m_inc) ac_st<MT>(a.inc, g, m_inc = c2.inc);
          if (c2.out != m_out) ac_st<MT>(a.out, g, m_out = c2.out);
          if (c2.lrn != m_lrn) ac_st<MT>(a.lrn, g, m_lrn = c2.lrn);
          if (c2.lnx != m_lnx) ac_st<MT>(a.lnx, g, m_lnx = c2.lnx);
          if (c2.isl != m_isl) ac_st<MT>(a.isl, g, m_isl = c2.isl);
          if (c2.trk != m_trk) ac_st<MT>(a.trk, g, m_trk = c2.trk);
          if (c2.al != c.al) a.auto_leave[g] = static_cast<uint8_t>(c2.al);
#pragma unroll
          for (int s = 0; s < S; s++) {
            const bool was = (c.trk >> s) & 1u, now = (c2.trk >> s) & 1u;
            if ((was && !now) || (now && (!was || id2[s] != id[s])))
              a.ids[static_cast<uint64_t>(s) * a.G + g] = now ? id2[s] : 0ull;
            // a slot that is not tracked holds no ID in registers
            id2[s] = now ? id2[s] : 0ull;
          }
          // p's view of the configuration where it is other memory
          if (a.p_inc) ac_st<MT>(a.p_inc, g, c2.inc);
          if (a.p_out) ac_st<MT>(a.p_out, g, c2.out);
          if (a.p_trk) ac_st<MT>(a.p_trk, g, c2.trk);
          // initProgress (:251-274): Match 0, Next = lastIndex, Probe,
          // RecentActive, empty Inflights
#pragma unroll
          for (int s = 0; s < S; s++) {
            if (((created >> s) & 1u) == 0) continue;
            const uint64_t k = static_cast<uint64_t>(s) * a.pstride + g;
            a.p_match[k] = 0;
            a.p_next[k] = li;
            a.p_pending[k] = 0;
            a.p_pw[k] = QE_PR_PROBE | QE_PF_RECENT_ACTIVE;
          }
          c = c2;
#pragma unroll
          for (int s = 0; s < kCCMax; s++) id[s] = id2[s];
        }
      }
      refused = res >= QE_AC_REFUSED;
    }
    ac_out<S, MT>(a, j, res, ccr, c, id, created);
  }
  if (led) a.switched[g] = 1;
}

// One lane per record, one wave per 64-record tile: the head test on the
// tile's group row and its predecessor (a dropped load for record 0), then the
// heads' walks.
template <int S>
__global__ __launch_bounds__(kBlock) void k_apply_conf(ACArgs a) {
  using MT = typename std::conditional<(S <= 8), uint8_t, uint16_t>::type;
  const uint64_t n = ac_records(a);
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(n, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const uint64_t r0 = t * 64;
    const uint32_t cnt = tile_n(n, t);
    const bool live = lane < cnt;
    const uint64_t gid = bld64<kNT>(mk_rsrc(a.group + r0, cnt * 8), lane * 8);
    // record r0 + lane - 1: the row from one record earlier on (none before record 0)
    const uint32_t back = r0 ? 1u : 0u;
    const bool has_prev = live && (lane + back) != 0;
    const uint64_t prev = bld64<kNT>(mk_rsrc(a.group + r0 - back, (cnt + back) * 8),
                                     has_prev ? (lane + back - 1u) * 8 : kOOB);
    if (live && (!has_prev || prev != gid)) ac_run<S, MT>(a, n, r0 + lane, gid, has_prev && gid < prev);
  }
}

#endif  // QE_APPLYCONF_KERNELS

}  // namespace qe
