// qe_carry.hpp — qe_carry: a list of sent records (a qe_outbox or qe_replies
// list: `group` the sender, `to` a slot of the sender) turned into the list the
// receivers' qe_inbox reads (`group` the receiver, `from` the sender's slot in
// the receiver's numbering), by the host's peer table, with the losses of the
// reference's in-process network (raft/raft_test.go:4633-4778: send, filter)
// and the MsgSnapStatus of node.ReportSnapshot (include/etcd_quorum.h states the
// rules; tests/carry_model.py restates them sequentially).
//
// A record's disposition depends on the record and the peer table alone, never
// on another record, so there is no key pass and no scratch word: the call is
// the routing layer's lanes and addressing (qe_route.hpp) in front of the
// record-list layer (qe_list.hpp), a source record as the layer's element.
//   k_carry_classify  one lane per record, one wave per 64-record tile of the
//                     source's CAPACITY (the launch is the host's, the length
//                     n = min(*count, capacity) the device's): disposition[i]
//                     for i < n, and for every i < capacity a count byte (the
//                     local records it yields, 0..2; 0 at or past n) and a
//                     remote flag byte into the scratch; the statistics.  The
//                     passes below run over the capacity and find nothing past n;
//   k_carry_count     list_count_block over the count bytes; k_collect_count
//                     over the remote flags; k_collect_scan for each;
//   k_carry_fill      the layer's walk.  A record yields a run of 0..2 local
//                     records, so the tile scans its lanes' counts (the
//                     qe_read_states shape: a lane stores its own run from tb +
//                     its prefix on); it gathers the source fields, the peer
//                     table and the E_in ent rows and stores the local records;
//   k_route_positions the routing layer's, over the remote flags.
// peer_group / peer_from / cut are addressed by the sender's g: 64-bit pointers
// under the lane's predicate (g - group_offset < G, to < S), as qe_route.hpp
// says.  Every store of a tile follows every load of it; every access is
// non-temporal; no atomics but the statistics; no LDS but the layer's.
// Bytes per source record: classify reads 10 (group, to, type) + 1 (drop) and,
// for a record that passes the checks, gathers 9 (+ 1 or 2 of cut), and writes
// 3; count and the flags' count read 2; the fill reads 1 and, per local record,
// 10 + 9 + 40 + 5 + 12 E_in and writes 55 + 12 E_out + 4 (src); the positions
// fill reads 1 and writes 4 per remote record.
#pragma once
#include "qe_route.hpp"

namespace qe {

constexpr uint64_t kCarrySalt = 0x8CB92BA72F3D8DD7ull;
constexpr uint32_t kCarryTileMax = 128;  // local records of one tile at most
// the types a link carries: 1..6 and 10..15
constexpr uint32_t kCarryTypes = QE_CARRY_TYPES;
static_assert(kCarryTypes == (0x7Eu | (0x3Fu << 10)), "QE_IMSG_APP .. _HEARTBEAT_RESP, _TRANSFER_LEADER .. _TIMEOUT_NOW");

struct CRArgs {
  uint64_t G, nb;  // the layer's: the source's capacity (its element is a source record), its chunks
  uint64_t ng, goff, stride;  // the batch
  uint32_t S, E_in, E_out, flags, ignore, cut_wide;
  // qe_peers
  const uint64_t *peer_group;
  const uint8_t *peer_from;
  // qe_carry_in
  const uint64_t *icount;
  const uint64_t *group;
  const uint8_t *to, *type;
  const uint64_t *term, *index, *log_term, *commit, *hint;
  const uint32_t *ctx;
  const uint8_t *mflags;
  const uint32_t *ent_len;
  const uint64_t *ent_term;
  const uint8_t *drop;
  const void *cut;
  // qe_carry_out
  uint64_t ocap, base, pitch;
  uint64_t *o_group;
  uint8_t *o_from, *o_type;
  uint64_t *o_term, *o_index, *o_log_term, *o_commit, *o_hint;
  uint32_t *o_ctx;
  uint8_t *o_mflags;
  uint32_t *o_ent_len;
  uint64_t *o_ent_term;
  uint32_t *o_src;
  uint8_t *disposition;
  // scratch
  uint8_t *kcnt, *rflag;  // [G]
  const uint64_t *offsets;
  uint32_t *counts;
  uint64_t *stats;
};

// defined in qe_inst_carry.hip
int dispatch_carry_classify(const CRArgs &a, hipStream_t st);
int dispatch_carry_count(const CRArgs &a, hipStream_t st);
int dispatch_carry_fill(const CRArgs &a, hipStream_t st);

#ifdef QE_ROUTE_KERNELS

// The list's length: every kernel reads it itself.
__device__ __forceinline__ uint64_t carry_n(const CRArgs &a) {
  const uint64_t c = *a.icount;
  return c < a.G ? c : a.G;
}

// The peer behind slot `to` of group g, for the lanes with `on` (the bounds
// check of the three gathers): QE_PEER_NONE / 0xFF for the others.
struct CarryPeer {
  uint64_t group;
  uint32_t from;
};
__device__ __forceinline__ CarryPeer carry_peer(const CRArgs &a, bool on, uint64_t g, uint32_t to) {
  CarryPeer p = {QE_PEER_NONE, 0xFFu};
  if (on) {
    const uint64_t k = to * a.stride + g;
    p.group = __builtin_nontemporal_load(a.peer_group + k);
    p.from = __builtin_nontemporal_load(a.peer_from + k);
  }
  return p;
}

enum { CR_GROUPS, CR_LOCAL, CR_REMOTE, CR_LOST, CR_BAD, CR_VIOL, CR_STATUS, CR_CSUM, CR_N };

// The classify pass: rules 1-5 as far as the counts go.
__global__ __launch_bounds__(kBlock) void k_carry_classify(CRArgs a) {
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(a.G, lane, wave, nwaves, ntiles);
  const uint64_t n = carry_n(a);
  const bool status = (a.flags & QE_CARRY_SNAP_STATUS) != 0;
  uint64_t cnt[CR_N] = {};
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    RouteRec r;  // (`from` holds the record's `to`)
    route_rec(r, a.group, a.to, a.type, n, a.goff, t, lane);
    const uint64_t r0 = t * 64;
    const uint32_t nl = tile_n(n, t), nc = tile_n(a.G, t);
    const uint32_t to = r.from;
    const bool dropped = bld8<kNT>(opt_rsrc(a.drop, r0, nl), lane) != 0;
    const bool typed = r.type < 32 && ((kCarryTypes >> r.type) & 1u);
    const bool in = r.live && typed && r.g < a.ng && to < a.S;
    // ---- the gathers, addressed by g ----
    const CarryPeer p = carry_peer(a, in, r.g, to);
    uint32_t cutm = 0;
    if (in && a.cut)
      cutm = a.cut_wide ? __builtin_nontemporal_load(static_cast<const uint16_t *>(a.cut) + r.g)
                        : __builtin_nontemporal_load(static_cast<const uint8_t *>(a.cut) + r.g);
    // ---- the disposition ----
    const bool here = p.group - a.goff < a.ng;
    const bool ok = in && p.group != QE_PEER_NONE && !(here && p.from >= a.S);
    const bool lost = ok && (((a.ignore >> r.type) & 1u) || dropped || ((cutm >> to) & 1u));
    const bool remote = ok && !lost && !here, local = ok && !lost && here;
    const bool snap = status && r.type == QE_IMSG_SNAP;
    const uint32_t disp = !ok ? QE_TD_BAD : lost ? QE_TD_LOST : here ? QE_TD_LOCAL : QE_TD_REMOTE;
    const uint32_t k = local ? (snap ? 2u : 1u) : (lost && snap) ? 1u : 0u;
    // ---- the stores ----
    bst8<kNT>(disp, mk_rsrc(a.disposition + r0, nl), lane);
    bst8<kNT>(k, mk_rsrc(a.kcnt + r0, nc), lane);
    bst8<kNT>(remote ? 1u : 0u, mk_rsrc(a.rflag + r0, nc), lane);
    if (a.stats) {
      const bool bad = r.live && !ok;
      cnt[CR_GROUPS] += k;
      cnt[CR_LOCAL] += local ? 1u : 0u;
      cnt[CR_REMOTE] += remote ? 1u : 0u;
      cnt[CR_LOST] += lost ? 1u : 0u;
      cnt[CR_BAD] += bad ? 1u : 0u;
      cnt[CR_VIOL] += bad ? 1u : 0u;
      cnt[CR_STATUS] += (snap && (local || lost)) ? 1u : 0u;
      cnt[CR_CSUM] += r.live ? route_hash(r.gid, kCarrySalt, disp, r.type, to, r.key - 1u) : 0u;
    }
  }
  if (a.stats) {
    const int idx[CR_N] = {QE_STAT_GROUPS,     QE_STAT_CARRY_LOCAL, QE_STAT_CARRY_REMOTE,
                           QE_STAT_CARRY_LOST, QE_STAT_CARRY_BAD,   QE_STAT_INVARIANT_VIOLATIONS,
                           QE_STAT_CARRY_SNAP_STATUS, QE_STAT_CHECKSUM};
    wave_stats_add<CR_N>(cnt, idx, a.stats);
  }
}

// The counts of the layer: a record's count byte.
struct CarryCounts {
  const uint8_t *kcnt;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const rsrc_t rk = mk_rsrc(kcnt + base, nc);
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) k[r] = bld8<kNT>(rk, list_elem(r));
  }
};

// The fields of a local record.
struct CarryRec {
  uint64_t group, term, index, log_term, commit, hint;
  uint32_t from, type, ctx, mflags;
  uint32_t el[QE_MAX_MSG_RUNS];
  uint64_t et[QE_MAX_MSG_RUNS];
};

// The output descriptors of one tile.
struct CarryOut {
  rsrc_t group, from, type, term, index, log_term, commit, hint, ctx, mflags, src;
  rsrc_t el[QE_MAX_MSG_RUNS], et[QE_MAX_MSG_RUNS];
};

// One record per lane with `on`, at position pos of the tile's room.
__device__ __forceinline__ void carry_emit(const CarryOut &d, uint32_t E_out, bool on, uint32_t pos,
                                           const CarryRec &c, uint32_t src) {
  const uint32_t p1 = on ? pos : kOOB, p4 = on ? pos * 4 : kOOB, p8 = on ? pos * 8 : kOOB;
  bst64<kNT>(c.group, d.group, p8);
  bst8<kNT>(c.from, d.from, p1);
  bst8<kNT>(c.type, d.type, p1);
  bst64<kNT>(c.term, d.term, p8);
  bst64<kNT>(c.index, d.index, p8);
  bst64<kNT>(c.log_term, d.log_term, p8);
  bst64<kNT>(c.commit, d.commit, p8);
  bst64<kNT>(c.hint, d.hint, p8);
  bst32<kNT>(c.ctx, d.ctx, p4);
  bst8<kNT>(c.mflags, d.mflags, p1);
#pragma unroll
  for (uint32_t j = 0; j < QE_MAX_MSG_RUNS; j++) {
    if (j < E_out) {  // (uniform)
      bst32<kNT>(c.el[j], d.el[j], p4);
      bst64<kNT>(c.et[j], d.et[j], p8);
    }
  }
  bst32<kNT>(src, d.src, p4);
}

// Tile t of the source, whose first local record has position tb behind `base`.
__device__ __forceinline__ void carry_tile(const CRArgs &a, uint64_t t, uint64_t tb, uint32_t lane,
                                           uint64_t (&)[1]) {
  const uint64_t r0 = t * 64;
  const uint32_t n = tile_n(carry_n(a), t);
  const bool status = (a.flags & QE_CARRY_SNAP_STATUS) != 0;
  // ---- 1. who yields what (a lane past n reads 0), the scan of the counts ----
  const uint32_t mine = bld8<kNT>(mk_rsrc(a.kcnt + r0, n), lane);
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= static_cast<uint32_t>(d)) inc += o;
  }
  const uint32_t pre = inc - mine;
  const bool has = mine != 0;
  const uint32_t h1 = has ? lane : kOOB, h8 = has ? lane * 8 : kOOB;
  // ---- 2. the source fields (a record with a count passed rule 1: g is in the
  //         batch and to < S) ----
  const uint64_t gid = bld64<kNT>(mk_rsrc(a.group + r0, n * 8), h8);
  const uint32_t to = bld8<kNT>(mk_rsrc(a.to + r0, n), h1);
  const uint32_t type = bld8<kNT>(mk_rsrc(a.type + r0, n), h1);
  // a lost MsgSnap yields its status record alone
  const bool rej = has && status && type == QE_IMSG_SNAP && mine == 1;
  const bool loc = has && !rej;
  const uint32_t l4 = loc ? lane * 4 : kOOB, l8 = loc ? lane * 8 : kOOB;
  CarryRec c;
  c.type = type;
  c.term = bld64<kNT>(mk_rsrc(a.term + r0, n * 8), l8);
  c.index = bld64<kNT>(mk_rsrc(a.index + r0, n * 8), l8);
  c.log_term = bld64<kNT>(mk_rsrc(a.log_term + r0, n * 8), l8);
  c.commit = bld64<kNT>(opt_rsrc(a.commit, r0, n), l8);
  c.hint = bld64<kNT>(opt_rsrc(a.hint, r0, n), l8);
  c.ctx = bld32<kNT>(opt_rsrc(a.ctx, r0, n), l4);
  c.mflags = bld8<kNT>(opt_rsrc(a.mflags, r0, n), loc ? lane : kOOB);
#pragma unroll
  for (uint32_t j = 0; j < QE_MAX_MSG_RUNS; j++) {
    c.el[j] = 0;
    c.et[j] = 0;
    if (j < a.E_in) {  // (uniform)
      const uint64_t row = j * a.G + r0;
      c.el[j] = bld32<kNT>(mk_rsrc(a.ent_len + row, n * 4), l4);
      c.et[j] = bld64<kNT>(mk_rsrc(a.ent_term + row, n * 8), l8);
    }
  }
  const CarryPeer p = carry_peer(a, loc, gid - a.goff, to);
  c.group = loc ? p.group : gid;
  c.from = loc ? p.from : to;
  c.type = rej ? QE_IMSG_SNAP_STATUS_REJECT : type;
  const CarryRec s = {gid, 0, 0, 0, 0, 0, to, QE_IMSG_SNAP_STATUS, 0, 0, {}, {}};
  // ---- 3. the stores: a lane's run from tb + pre on; capacity is the
  //         descriptors' ----
  const auto [tbc, rem] = list_room(a.base + tb, a.ocap, kCarryTileMax);
  CarryOut d;
  d.group = mk_rsrc(a.o_group + tbc, rem * 8);
  d.from = mk_rsrc(a.o_from + tbc, rem);
  d.type = mk_rsrc(a.o_type + tbc, rem);
  d.term = mk_rsrc(a.o_term + tbc, rem * 8);
  d.index = mk_rsrc(a.o_index + tbc, rem * 8);
  d.log_term = mk_rsrc(a.o_log_term + tbc, rem * 8);
  d.commit = mk_rsrc(a.o_commit + tbc, rem * 8);
  d.hint = mk_rsrc(a.o_hint + tbc, rem * 8);
  d.ctx = opt_rsrc(a.o_ctx, tbc, rem);
  d.mflags = opt_rsrc(a.o_mflags, tbc, rem);
  d.src = opt_rsrc(a.o_src, tbc, rem);
#pragma unroll
  for (uint32_t j = 0; j < QE_MAX_MSG_RUNS; j++) {
    const bool row = j < a.E_out;
    d.el[j] = row ? mk_rsrc(a.o_ent_len + j * a.pitch + tbc, rem * 4) : mk_rsrc(a.o_ent_len, 0);
    d.et[j] = row ? mk_rsrc(a.o_ent_term + j * a.pitch + tbc, rem * 8) : mk_rsrc(a.o_ent_term, 0);
  }
  const uint32_t src = static_cast<uint32_t>(r0) + lane;
  carry_emit(d, a.E_out, has, pre, c, src);
  if (__builtin_amdgcn_ballot_w64(mine == 2)) carry_emit(d, a.E_out, mine == 2, pre + 1, s, src);
}

__global__ __launch_bounds__(kBlock) void k_carry_count(CRArgs a) {
  list_count_block(a.G, a.counts, CarryCounts{a.kcnt});
}

// The count bytes at or past n are 0; the classify pass holds the statistics
// (the dispatcher passes none).
__global__ __launch_bounds__(kBlock) void k_carry_fill(CRArgs a) {
  const int idx[1] = {QE_STAT_GROUPS};
  list_fill_walk<carry_tile>(a, idx, CarryCounts{a.kcnt});
}
#endif  // QE_ROUTE_KERNELS

}  // namespace qe
