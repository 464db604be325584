// qe_readstates.hpp — qe_read_note and qe_read_states: the answers to ReadIndex
// requests as a dense, ordered list of records (include/etcd_quorum.h states
// the rules).
//
// readOnly keeps, per pending request, the read index and the request itself
// (readIndexStatus{req, index}, raft/read_only.go:29-37); advance hands the
// released ones back in queue order (:85-112) and responseToReadIndexReq
// (raft/raft.go:1737-1751) turns each into a local ReadState or a
// MsgReadIndexResp to req.From.  The queue (qe_progress.read_*) holds the acks
// and the key; the book (qe_read_book) holds the index and the origin, at the
// same address: context c of group g at [g * cap + c % cap].
//
// qe_read_states is the three passes of the record-list layer (qe_list.hpp):
// k_read_states_count and k_read_states_fill.  The counts read only bytes:
// read_released + (term_commit != 0) + (ri_result == QE_RI_RESPOND).  Unlike
// its siblings a group here has 0..257 records, not one per (kind, slot) at
// most: a tile scans its lanes' counts (a wave scan, no LDS), lane g owns the
// positions tb + prefix[g] .. and walks its released requests j = 0 .. k - 1
// under the ballot of the lanes that still have one, the book and key loads
// of round j going through range-checked descriptors.  Every store follows
// every load of the tile's header; the book loads of round j follow the
// stores of round j - 1, which is fine: nothing resident is written.
//
// qe_read_note is elementwise, a thread per group.  Nothing here depends on
// the slot count at compile time: one object (qe_inst_readstates.hip).
#pragma once
#include "qe_list.hpp"

namespace qe {

constexpr uint32_t kRsTileMax = 64 * (QE_READ_CAP_MAX + 2);  // records of one tile at most
constexpr uint64_t kReadStatesSalt = 0xE7037ED1A0B428DBull;

struct RSArgs {
  uint64_t G, goff;
  uint32_t S;
  uint32_t cap;  // entries of a group in the book and in read_keys
  uint64_t nb;   // chunks
  // qe_read_states_in
  const uint8_t *read_released, *term_commit;
  const uint64_t *term_commit_index;
  const uint8_t *ri_result;
  const uint64_t *ri_index;
  const uint8_t *ri_from;
  const uint64_t *ri_key;
  // qe_progress
  const uint32_t *read_head;
  const uint8_t *self_slot;
  const uint64_t *read_keys;
  // qe_read_book
  const uint64_t *req_index;
  const uint8_t *req_from;
  // qe_read_states_out
  uint64_t ocap;
  uint64_t *o_group;
  uint8_t *o_kind, *o_to;
  uint32_t *o_ctx;
  uint64_t *o_index, *o_key;
  // scratch
  const uint64_t *offsets;
  uint32_t *counts;
  uint64_t *stats;
};

struct RNoteArgs {
  uint64_t G;
  uint32_t cap;
  const uint8_t *result;
  const uint32_t *ctx;
  const uint64_t *index;
  const uint8_t *from;
  uint64_t *req_index;
  uint8_t *req_from;
};

// defined in qe_inst_readstates.hip
int dispatch_read_note(const RNoteArgs &a, hipStream_t st);
int dispatch_read_states_count(const RSArgs &a, hipStream_t st);
int dispatch_read_states_fill(const RSArgs &a, hipStream_t st);

// The counts of the layer, from bytes alone; an absent row reads 0 through
// the null descriptor.
struct ReadStatesCounts {
  const RSArgs &a;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const rsrc_t rr = opt_rsrc(a.read_released, base, nc), rt = opt_rsrc(a.term_commit, base, nc),
                 ri = opt_rsrc(a.ri_result, base, nc);
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) {
      const uint32_t i = list_elem(r);
      k[r] = bld8<kNT>(rr, i) + (bld8<kNT>(rt, i) != 0 ? 1u : 0u) +
             (bld8<kNT>(ri, i) == QE_RI_RESPOND ? 1u : 0u);
    }
  }
};

enum { RS_GROUPS, RS_STATE, RS_RESP, RS_TC, RS_CSUM, RS_N };

// The output descriptors of one tile.
struct RSOut {
  rsrc_t group, kind, to, ctx, index, key;
};

// responseToReadIndexReq's choice: req.From == None || req.From == r.id.
__device__ __forceinline__ bool rs_local(uint32_t from, uint32_t self, uint32_t S) {
  return from >= S || from == self;
}

// One record per lane with `bit`, at position pos.
__device__ __forceinline__ void rs_emit(const RSOut &d, bool stats, bool bit, uint32_t pos,
                                        uint64_t gid, uint32_t kind, uint32_t to, uint32_t ctx,
                                        uint64_t index, uint64_t key, uint64_t (&cnt)[RS_N]) {
  const uint32_t p1 = bit ? pos : kOOB, p4 = bit ? pos * 4 : kOOB, p8 = bit ? pos * 8 : kOOB;
  bst64<kNT>(gid, d.group, p8);
  bst8<kNT>(kind, d.kind, p1);
  bst8<kNT>(to, d.to, p1);
  bst32<kNT>(ctx, d.ctx, p4);
  bst64<kNT>(index, d.index, p8);
  bst64<kNT>(key, d.key, p8);
  if (stats) {
    uint64_t h = mix64((gid * kPhi) ^ kReadStatesSalt ^ (static_cast<uint64_t>(kind) << 56) ^
                       (static_cast<uint64_t>(to) << 48) ^ ctx);
    h = mix64(h ^ index);
    h = mix64(h ^ key);
    cnt[RS_STATE] += (bit && kind == QE_RS_STATE) ? 1u : 0u;
    cnt[RS_RESP] += (bit && kind == QE_RS_RESP) ? 1u : 0u;
    cnt[RS_TC] += (bit && kind == QE_RS_TERM_COMMIT) ? 1u : 0u;
    cnt[RS_CSUM] += bit ? h : 0u;
  }
}

// Tile t, whose first record has position tb.
__device__ __forceinline__ void read_states_tile(const RSArgs &a, uint64_t t, uint64_t tb,
                                                 uint32_t lane, uint64_t (&cnt)[RS_N]) {
  const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
  const bool stats = a.stats != nullptr;
  const uint32_t S = a.S, cap = a.cap;
  // ---- 1. who has what (a lane past n reads 0) ----
  const uint32_t k = bld8<kNT>(opt_rsrc(a.read_released, g0, n), lane);
  const bool tc = bld8<kNT>(opt_rsrc(a.term_commit, g0, n), lane) != 0;
  const bool im = bld8<kNT>(opt_rsrc(a.ri_result, g0, n), lane) == QE_RI_RESPOND;
  const uint32_t mine = k + (tc ? 1u : 0u) + (im ? 1u : 0u);
  // the exclusive scan of the lanes' counts: lane g owns tb + pre .. + mine - 1
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= static_cast<uint32_t>(d)) inc += o;
  }
  const uint32_t pre = inc - mine;
  // ---- 2. the header rows, under the ballot of the lanes that need them ----
  const bool rel = k != 0, need_self = rel || im;
  uint32_t head = 0, self = 0xFFu;
  if (__builtin_amdgcn_ballot_w64(rel))
    head = bld32<kNT>(mk_rsrc(a.read_head + g0, n * 4), rel ? lane * 4 : kOOB);
  if (a.self_slot && __builtin_amdgcn_ballot_w64(need_self))
    self = bld8<kNT>(mk_rsrc(a.self_slot + g0, n), need_self ? lane : kOOB);
  self = need_self ? self : 0xFFu;
  uint64_t tci = 0;
  if (__builtin_amdgcn_ballot_w64(tc))
    tci = bld64<kNT>(mk_rsrc(a.term_commit_index + g0, n * 8), tc ? o8 : kOOB);
  uint32_t i_from = 0xFFu;
  uint64_t i_idx = 0, i_key = 0;
  if (__builtin_amdgcn_ballot_w64(im)) {
    i_idx = bld64<kNT>(mk_rsrc(a.ri_index + g0, n * 8), im ? o8 : kOOB);
    if (a.ri_from) i_from = bld8<kNT>(mk_rsrc(a.ri_from + g0, n), im ? lane : kOOB);
    i_from = im ? i_from : 0xFFu;
    i_key = bld64<kNT>(opt_rsrc(a.ri_key, g0, n), im ? o8 : kOOB);
  }
  // ---- 3. the records ----
  // what of the arrays this tile may write: capacity is the descriptors'
  const auto [tbc, rem] = list_room(tb, a.ocap, kRsTileMax);
  const RSOut d = {mk_rsrc(a.o_group + tbc, rem * 8), mk_rsrc(a.o_kind + tbc, rem),
                   mk_rsrc(a.o_to + tbc, rem),        mk_rsrc(a.o_ctx + tbc, rem * 4),
                   mk_rsrc(a.o_index + tbc, rem * 8),
                   a.o_key ? mk_rsrc(a.o_key + tbc, rem * 8) : mk_rsrc(a.o_key, 0)};
  // the released requests, oldest first: contexts head - k + j
  if (__builtin_amdgcn_ballot_w64(rel)) {
    // the tile's rows of the book and of the keys: [64][cap]
    const rsrc_t b_idx = a.req_index ? mk_rsrc(a.req_index + g0 * cap, n * cap * 8)
                                     : mk_rsrc(a.req_index, 0);
    const rsrc_t b_from = a.req_from ? mk_rsrc(a.req_from + g0 * cap, n * cap)
                                     : mk_rsrc(a.req_from, 0);
    const rsrc_t b_key = a.read_keys ? mk_rsrc(a.read_keys + g0 * cap, n * cap * 8)
                                     : mk_rsrc(a.read_keys, 0);
    const uint32_t first = head - k;
    for (uint32_t j = 0; __builtin_amdgcn_ballot_w64(j < k); j++) {  // (the tile's maximum)
      const bool on = j < k;
      const uint32_t c = first + j;
      const uint32_t e = lane * cap + c % cap;
      const uint64_t idx = bld64<kNT>(b_idx, on ? e * 8 : kOOB);
      const uint32_t f = bld8<kNT>(b_from, on ? e : kOOB);
      const uint64_t key = bld64<kNT>(b_key, on ? e * 8 : kOOB);
      const bool local = rs_local(f, self, S);
      rs_emit(d, stats, on, pre + j, gid, local ? QE_RS_STATE : QE_RS_RESP, local ? 0xFFu : f, c,
              idx, key, cnt);
    }
  }
  // releasePendingReadIndexMessages fired
  if (__builtin_amdgcn_ballot_w64(tc))
    rs_emit(d, stats, tc, pre + k, gid, QE_RS_TERM_COMMIT, 0xFFu, 0u, tci, 0, cnt);
  // the immediate answer of a qe_read_index
  if (__builtin_amdgcn_ballot_w64(im)) {
    const bool local = rs_local(i_from, self, S);
    rs_emit(d, stats, im, pre + k + (tc ? 1u : 0u), gid, local ? QE_RS_STATE : QE_RS_RESP,
            local ? 0xFFu : i_from, 0u, i_idx, i_key, cnt);
  }
  cnt[RS_GROUPS] += mine != 0 ? 1u : 0u;
}

}  // namespace qe
