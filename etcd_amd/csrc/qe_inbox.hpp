// qe_inbox.hpp — qe_inbox: a list of delivered messages routed into the
// message rows of the step entry points (include/etcd_quorum.h states the
// rules; tests/inbox_model.py restates them sequentially).
//
// The sequential rule (per group, walk the records in list order: the first
// opens the wave, a response joins a wave of responses unless its slot is
// taken, anything else closes the group) has an exact order-free form.  The
// key of record i is i + 1; key 0 is the virtual MsgHup of a tick.  Four kinds
// of scratch word per group (qe_route.hpp: all-ones = none, each the result of
// 32-bit atomicMin, so any arrival order gives the same bit-exact outputs):
//   first[g]    lowest key of any valid record of g;
//   cell[s][g]  lowest key of a class-R record of g with from = s;
//   stop[g]     lowest key that ends the wave: a record other than first[g]
//               that is not class R, or is class R but not its cell's minimum
//               (an earlier response of the same slot exists, and it is in the
//               wave because every key below stop[g] is); a non-R opener puts
//               its own key here, a tick HUP puts 0;
//   hi[g]       lowest key of a higher-term class-R record that is its cell's
//               minimum.
// A record is in its group's wave iff it is the non-R opener (key ==
// first[g]) or is class R with key < stop[g]; the STEPDOWN record is hi[g]
// where that is in the wave.
//
// Kernels, ordered by kernel boundaries alone (no spin wait, no look-back:
// DESIGN.md §8 item 3):
//   k_inbox_init   G-sized: the scratch words, the empty type rows, the tick HUPs;
//   k_inbox_p1     first and cell;
//   k_inbox_p2     stop and hi (reads f->term);
//   k_inbox_p3     dispositions, the scatter into the rows, one deferred flag
//                  byte per record, the statistics;
//   k_collect_count / k_collect_scan (qe_collect.hpp) over the flags, then the
//   routing layer's k_route_positions: the positions of the flagged records.
// The lanes, the tiles and the addressing are the routing layer's.  In pass 3
// nobody reads cell[][]: with statistics, cell[0][g] is the group's "counted"
// mark (atomicExch: exactly one ROUTED response per group sees it unmarked).
#pragma once
#include "qe_route.hpp"

namespace qe {

constexpr uint64_t kInboxSalt = 0xD1B54A32D192ED03ull;
constexpr uint32_t kIbMarked = 0xFFFFFFFEu;  // cell[0][g] in pass 3: the group is counted
enum : uint32_t { IB_BAD = 0, IB_F, IB_S, IB_R, IB_V };

struct IBArgs {
  uint64_t G, goff, stride, n;
  uint32_t S, E;
  // qe_follower
  const uint64_t *fterm;
  const uint8_t *fstate;
  // qe_inbox_in
  const uint64_t *group;
  const uint8_t *from, *type;
  const uint64_t *term, *index, *log_term, *commit, *hint;
  const uint32_t *ctx;
  const uint8_t *flags;
  const uint32_t *ent_len;
  const uint64_t *ent_term;
  const uint8_t *tick;
  // qe_inbox_out
  uint8_t *f_type, *f_from;
  uint64_t *f_term, *f_index, *f_log_term, *f_commit;
  uint32_t *f_ent_len;
  uint64_t *f_ent_term;
  uint8_t *s_type, *s_from;
  uint64_t *s_term, *s_snap_index, *s_snap_term;
  uint8_t *v_type, *v_from;
  uint64_t *v_term, *v_index, *v_log_term;
  uint8_t *v_flags;
  uint8_t *r_type;
  uint64_t *r_index, *r_hint, *r_log_term;
  uint32_t *r_ctx;
  uint32_t *f_src, *s_src, *v_src, *r_src;
  uint8_t *disposition;
  uint64_t *stats;
  // scratch
  uint32_t *first, *stop, *hi, *cell;  // [G], [G], [G], [S][G]
  uint8_t *dflag;                      // [n]
};

// defined in qe_inst_route.hip
int dispatch_inbox_init(const IBArgs &a, hipStream_t st);
int dispatch_inbox_passes(const IBArgs &a, hipStream_t st);

#ifdef QE_ROUTE_KERNELS

__device__ __forceinline__ uint32_t inbox_class(uint32_t type) {
  if (type == QE_IMSG_APP || type == QE_IMSG_HEARTBEAT) return IB_F;
  if (type == QE_IMSG_SNAP) return IB_S;
  if (type >= QE_IMSG_APP_RESP && type <= QE_IMSG_TRANSFER_LEADER) return IB_R;
  if (type >= QE_IMSG_VOTE && type <= QE_IMSG_HUP) return IB_V;
  return IB_BAD;
}

// Record `lane` of tile t: its head, its class and whether it takes part (rule 2).
struct IRec : RouteRec {
  uint32_t cls;
  bool valid;
};
__device__ __forceinline__ IRec inbox_rec(const IBArgs &a, uint64_t t, uint32_t lane) {
  IRec r;
  route_rec(r, a.group, a.from, a.type, a.n, a.goff, t, lane);
  r.cls = inbox_class(r.type);
  r.valid = r.live && r.g < a.G && r.cls != IB_BAD && (r.from < a.S || r.type == QE_IMSG_HUP);
  return r;
}

// The init pass, one thread per group: the scratch words, the complete type
// rows and the virtual HUP of a tick (rule 4).
__global__ __launch_bounds__(kBlock) void k_inbox_init(IBArgs a) {
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g < a.G;
       g += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const bool hup = a.tick && (a.tick[g] & QE_TICK_HUP);
    a.first[g] = hup ? 0u : kRouteNone;
    a.stop[g] = hup ? 0u : kRouteNone;
    a.hi[g] = kRouteNone;
    for (uint32_t s = 0; s < a.S; s++) {
      a.cell[s * a.G + g] = kRouteNone;
      a.r_type[s * a.stride + g] = QE_MSG_NONE;
    }
    a.f_type[g] = QE_LMSG_NONE;
    a.s_type[g] = QE_SMSG_NONE;
    a.v_type[g] = hup ? QE_VMSG_HUP : QE_VMSG_NONE;
    if (hup) {
      a.v_from[g] = 0;
      a.v_term[g] = 0;
      a.v_index[g] = 0;
      a.v_log_term[g] = 0;
      if (a.v_flags) a.v_flags[g] = 0;
      if (a.v_src) a.v_src[g] = QE_INBOX_SRC_TICK;
    }
  }
}

// Pass 1: first and cell.
__global__ __launch_bounds__(kBlock) void k_inbox_p1(IBArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.n, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const IRec r = inbox_rec(a, t, lane);
    if (r.valid) {
      atomicMin(a.first + r.g, r.key);
      if (r.cls == IB_R) atomicMin(a.cell + r.from * a.G + r.g, r.key);
    }
  }
}

// Whether a response's term is above the receiver's (rule 6a, 6c).
__device__ __forceinline__ bool higher_term(uint64_t mterm, uint64_t rterm) {
  return mterm != 0 && mterm > rterm;
}

// Pass 2: stop and hi.
__global__ __launch_bounds__(kBlock) void k_inbox_p2(IBArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.n, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const IRec r = inbox_rec(a, t, lane);
    const uint32_t cnt = tile_n(a.n, t);
    const bool isr = r.valid && r.cls == IB_R;
    const uint64_t mterm = bld64<kNT>(mk_rsrc(a.term + t * 64, cnt * 8), isr ? lane * 8 : kOOB);
    if (r.valid) {
      const bool opener = a.first[r.g] == r.key;
      const bool cmin = isr && a.cell[r.from * a.G + r.g] == r.key;
      if (opener ? !isr : !cmin) atomicMin(a.stop + r.g, r.key);
      if (cmin && higher_term(mterm, a.fterm[r.g])) atomicMin(a.hi + r.g, r.key);
    }
  }
}

enum { I_GROUPS, I_ROUTED, I_STEPDOWN, I_DEFERRED, I_LOWER, I_NOTLEAD, I_BAD, I_VIOL, I_CSUM, I_N };

// Pass 3: the dispositions, the rows, the deferred flags.
template <int E>
__global__ __launch_bounds__(kBlock) void k_inbox_p3(IBArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.n, lane, wave, nwaves, ntiles);
  uint64_t cnt[I_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const IRec r = inbox_rec(a, t, lane);
    const uint64_t r0 = t * 64;
    const uint32_t n = tile_n(a.n, t);
    const uint32_t pos = r.key - 1u;
    // ---- the wave, the preamble ----
    const bool isr = r.valid && r.cls == IB_R;
    uint32_t first = kRouteNone, stop = 0, hi = kRouteNone, state = 0;
    uint64_t rterm = 0;
    if (r.valid) {
      first = a.first[r.g];
      stop = a.stop[r.g];
      if (isr) {
        hi = a.hi[r.g];
        rterm = a.fterm[r.g];
        state = a.fstate[r.g];
      }
    }
    const bool member = r.valid && (isr ? r.key < stop : r.key == first);
    const uint32_t o8 = member ? lane * 8 : kOOB;
    const uint64_t mterm = bld64<kNT>(mk_rsrc(a.term + r0, n * 8), o8);
    uint32_t disp = QE_ID_BAD;
    if (r.valid) {
      disp = QE_ID_DEFERRED;
      if (member && !isr) disp = QE_ID_ROUTED;
      if (member && isr) {
        if (mterm != 0 && mterm < rterm)
          disp = QE_ID_DROP_LOWER_TERM;
        else if (higher_term(mterm, rterm))
          disp = hi == r.key ? QE_ID_STEPDOWN : QE_ID_DEFERRED;
        else
          disp = state != QE_STATE_LEADER ? QE_ID_DROP_NOT_LEADER : QE_ID_ROUTED;
      }
    }
    const bool routed = disp == QE_ID_ROUTED, down = disp == QE_ID_STEPDOWN;
    // ---- the fields of the records that go into a row ----
    const uint32_t w8 = routed ? lane * 8 : kOOB;
    const uint64_t index = bld64<kNT>(mk_rsrc(a.index + r0, n * 8), w8);
    const uint64_t lterm = bld64<kNT>(mk_rsrc(a.log_term + r0, n * 8), w8);
    const bool rf = routed && r.cls == IB_F, rs = routed && r.cls == IB_S;
    const bool rv = routed && r.cls == IB_V, rr = routed && r.cls == IB_R;
    const uint64_t commit = bld64<kNT>(mk_rsrc(a.commit + r0, n * 8), rf ? lane * 8 : kOOB);
    const uint64_t hint = bld64<kNT>(mk_rsrc(a.hint + r0, n * 8), rr ? lane * 8 : kOOB);
    const uint32_t ctx = bld32<kNT>(opt_rsrc(a.ctx, r0, n), rr ? lane * 4 : kOOB);
    const uint32_t vfl = bld8<kNT>(opt_rsrc(a.flags, r0, n), rv ? lane : kOOB);
    const bool app = rf && r.type == QE_IMSG_APP;
    uint32_t el[E > 0 ? E : 1] = {};
    uint64_t et[E > 0 ? E : 1] = {};
    if constexpr (E > 0) {
      if (__builtin_amdgcn_ballot_w64(app)) {
#pragma unroll
        for (int k = 0; k < E; k++) {
          const uint64_t row = static_cast<uint64_t>(k) * a.n + r0;
          el[k] = bld32<kNT>(mk_rsrc(a.ent_len + row, n * 4), app ? lane * 4 : kOOB);
          et[k] = bld64<kNT>(mk_rsrc(a.ent_term + row, n * 8), app ? lane * 8 : kOOB);
        }
      }
    }
    // ---- the stores (every one after every load of the tile) ----
    bst8<kNT>(disp, mk_rsrc(a.disposition + r0, n), lane);
    bst8<kNT>(disp == QE_ID_DEFERRED ? 1u : 0u, mk_rsrc(a.dflag + r0, n), lane);
    const uint64_t g = r.g;
    if (rf) {
      a.f_type[g] = r.type == QE_IMSG_APP ? QE_LMSG_APP : QE_LMSG_HEARTBEAT;
      a.f_from[g] = static_cast<uint8_t>(r.from);
      a.f_term[g] = mterm;
      a.f_index[g] = index;
      a.f_log_term[g] = lterm;
      a.f_commit[g] = commit;
      if (a.f_src) a.f_src[g] = pos;
      if constexpr (E > 0) {
        if (app) {
#pragma unroll
          for (int k = 0; k < E; k++) {
            a.f_ent_len[k * a.stride + g] = el[k];
            a.f_ent_term[k * a.stride + g] = et[k];
          }
        }
      }
    }
    if (rs) {
      a.s_type[g] = QE_SMSG_SNAP;
      a.s_from[g] = static_cast<uint8_t>(r.from);
      a.s_term[g] = mterm;
      a.s_snap_index[g] = index;
      a.s_snap_term[g] = lterm;
      if (a.s_src) a.s_src[g] = pos;
    }
    if (rv || down) {
      // QE_IMSG_VOTE .. _PREVOTE_RESP are QE_VMSG_* + 10; TIMEOUT_NOW and HUP swap
      const uint32_t vt = r.type == QE_IMSG_HUP ? QE_VMSG_HUP
                          : r.type == QE_IMSG_TIMEOUT_NOW ? QE_VMSG_TIMEOUT_NOW
                                                          : r.type - 10u;
      a.v_type[g] = down ? QE_VMSG_VOTE_RESP : vt;
      a.v_from[g] = static_cast<uint8_t>(r.from);
      a.v_term[g] = mterm;
      a.v_index[g] = down ? 0 : index;
      a.v_log_term[g] = down ? 0 : lterm;
      if (a.v_flags) a.v_flags[g] = down ? QE_VMF_REJECT : static_cast<uint8_t>(vfl);
      if (a.v_src) a.v_src[g] = pos;
    }
    if (rr) {
      const uint64_t k = r.from * a.stride + g;
      a.r_type[k] = static_cast<uint8_t>(r.type - 3u);
      a.r_index[k] = index;
      a.r_hint[k] = hint;
      a.r_log_term[k] = lterm;
      if (a.r_ctx) a.r_ctx[k] = ctx;
      if (a.r_src) a.r_src[k] = pos;
    }
    if (a.stats) {
      // one ROUTED record per group counts it: the opener of another class, or
      // the response that finds cell[0][g] unmarked
      bool counts = routed && !rr;
      if (rr) counts = atomicExch(a.cell + g, kIbMarked) != kIbMarked;
      const bool bad = r.live && !r.valid;
      cnt[I_GROUPS] += counts ? 1u : 0u;
      cnt[I_ROUTED] += routed ? 1u : 0u;
      cnt[I_STEPDOWN] += down ? 1u : 0u;
      cnt[I_DEFERRED] += disp == QE_ID_DEFERRED ? 1u : 0u;
      cnt[I_LOWER] += disp == QE_ID_DROP_LOWER_TERM ? 1u : 0u;
      cnt[I_NOTLEAD] += disp == QE_ID_DROP_NOT_LEADER ? 1u : 0u;
      cnt[I_BAD] += bad ? 1u : 0u;
      cnt[I_VIOL] += bad ? 1u : 0u;
      cnt[I_CSUM] += r.live ? route_hash(r.gid, kInboxSalt, disp, r.type, r.from, pos) : 0u;
    }
  }
  if (a.stats) {
    const int idx[I_N] = {QE_STAT_GROUPS,           QE_STAT_INBOX_ROUTED,
                          QE_STAT_INBOX_STEPDOWN,   QE_STAT_INBOX_DEFERRED,
                          QE_STAT_INBOX_LOWER_TERM, QE_STAT_INBOX_NOT_LEADER,
                          QE_STAT_INBOX_BAD,        QE_STAT_INVARIANT_VIOLATIONS,
                          QE_STAT_CHECKSUM};
    wave_stats_add<I_N>(cnt, idx, a.stats);
  }
}

#endif  // QE_ROUTE_KERNELS

}  // namespace qe
