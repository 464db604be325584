// qe_outbox.hpp — qe_outbox: the messages one leader-side call sent, as a
// dense, ordered list of records (include/etcd_quorum.h states the rules).
//
// The step kernels report a send as mask bits; maybeSendAppend
// (raft/raft.go:432-492) and bcastHeartbeatWithCtx (:525-532) say what the
// message of a bit carries.  Everything a record needs is resident: the masks,
// msg_index or Next, the term-run log, committed, the sender's term.
//
// Three passes over 4096-group chunks (64 tiles, a block of four waves each):
//   count   k_outbox_count: the records of a chunk, from the masks alone;
//   scan    k_collect_scan (qe_collect.hpp, launched by qe_outbox): the chunk
//           offsets and the total;
//   fill    k_outbox_fill: a block recounts its chunk's tiles from the mask
//           bytes (64 words of LDS, the only LDS here), a wave scans them, and
//           wave w writes the tiles 4k + w.  No block waits for another.
// A tile in the house idiom (qe_step.hpp): one lane per group; the masks, then
// term, the log's header and run table, snap_index and hb_ctx once per tile
// under the ballot of the lanes that need them; then the per-slot rows (index,
// or peer and next_before / next; hb_commit) of every slot in the tile's mask
// union; then, slot by slot, the records.  The records of a slot take
// consecutive positions in lane order (ballot + mbcnt; the slot's base is the
// popcount of the earlier slots' ballots), so a wave's stores for one slot are
// one contiguous run.  Every store follows every load of the tile.  Capacity is
// the output descriptors' num_records: a record past it is an out-of-range
// store, dropped, with no branch.  Every access is non-temporal.
//
// RM is the run-capacity bucket (log_runs <= 4 / 8 / 16, as k_compact), E the
// message's run capacity (qe_outbox_out.msg_runs).  The slot count and the mask
// width are run-time values: one object, not one per QE_S.
#pragma once
#include "qe_step.hpp"

namespace qe {

constexpr uint32_t kObRounds = 16;                    // groups per thread and chunk
constexpr uint32_t kObChunk = kBlock * kObRounds;     // groups per chunk (qe_collect's)
constexpr uint32_t kObTiles = kObChunk / 64;          // tiles per chunk
constexpr uint32_t kObTileMax = 64 * QE_MAX_SLOTS;    // records of one tile at most
constexpr uint64_t kOutboxSalt = 0xC2B2AE3D27D4EB4Full;

struct OBArgs {
  uint64_t G, goff, stride;
  uint32_t R, S;
  uint32_t wide;         // the masks are 16-bit words
  uint32_t max_entries;
  uint64_t nb;           // chunks
  const void *sent, *snap, *hb_sent;
  // qe_progress
  const uint64_t *committed, *last_index, *run_first, *run_term;
  const uint8_t *run_count;
  const uint64_t *next;
  const uint32_t *peer;
  const uint64_t *snap_src;  // snap_index, or first_index with snap_sub 1
  uint64_t snap_sub;
  // qe_outbox_in
  const uint64_t *index, *next_before, *term, *snap_term, *hb_commit;
  const uint32_t *hb_ctx;
  // qe_outbox_out
  uint64_t cap;
  uint64_t *o_group;
  uint8_t *o_to, *o_type;
  uint64_t *o_term, *o_index, *o_log_term, *o_commit;
  uint32_t *o_ctx, *o_ent_len;
  uint64_t *o_ent_term;
  // scratch
  const uint64_t *offsets;
  uint32_t *counts;
  uint64_t *stats;
};

// defined in qe_inst_outbox.hip
int dispatch_outbox_count(const OBArgs &a, hipStream_t st);
int dispatch_outbox_fill(const OBArgs &a, uint32_t msg_runs, hipStream_t st);

// `cnt` elements of a mask-typed array from element `first` on (NULL: reads 0).
__device__ __forceinline__ rsrc_t ob_mask_rsrc(const void *p, uint64_t first, uint32_t cnt,
                                               uint32_t sz) {
  return p ? mk_rsrc(static_cast<const uint8_t *>(p) + first * sz, cnt * sz) : mk_rsrc(p, 0);
}
__device__ __forceinline__ uint32_t ob_ld_mask(rsrc_t r, uint32_t i, bool wide) {
  return wide ? bld16<kNT>(r, i * 2) : bld8<kNT>(r, i);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ uint32_t lane_rank(uint64_t bal) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u));
}

// The records of each tile of chunk c into tcnt[kObTiles]: thread t takes the
// groups r * kBlock + t, so round r of wave w is tile 4r + w; the rounds'
// loads are independent and in flight together.
__device__ __forceinline__ void chunk_tile_counts(const OBArgs &a, bool wide, uint64_t c,
                                                  uint32_t *tcnt) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t base = c * kObChunk;
  const uint32_t nc = static_cast<uint32_t>(a.G - base < kObChunk ? a.G - base : kObChunk);
  const uint32_t sz = wide ? 2u : 1u, full = (1u << a.S) - 1u;
  const rsrc_t rs = ob_mask_rsrc(a.sent, base, nc, sz), rp = ob_mask_rsrc(a.snap, base, nc, sz),
               rh = ob_mask_rsrc(a.hb_sent, base, nc, sz);
  uint32_t m[kObRounds];
#pragma unroll
  for (uint32_t r = 0; r < kObRounds; r++) {
    const uint32_t i = r * kBlock + tid;  // past nc: out of range, reads 0
    m[r] = ob_ld_mask(rs, i, wide) | ob_ld_mask(rp, i, wide) | ob_ld_mask(rh, i, wide);
  }
#pragma unroll
  for (uint32_t r = 0; r < kObRounds; r++) {
    const uint32_t s = wave_sum_u32(popc(m[r] & full));
    if (lane == 0) tcnt[r * (kBlock / 64) + w] = s;
  }
}

// One block per chunk.  WIDE: the masks are 16-bit words.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_outbox_count(OBArgs a) {
  __shared__ uint32_t tcnt[kObTiles];
  chunk_tile_counts(a, WIDE, blockIdx.x, tcnt);
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t s = wave_sum_u32(tcnt[threadIdx.x]);
    if (threadIdx.x == 0) a.counts[blockIdx.x] = s;
  }
}

enum { O_GROUPS, O_APP, O_SNAP, O_HB, O_BAD, O_VIOL, O_ENTRIES, O_CSUM, O_N };

// Tile t, whose first record has position tb.
template <int RM, int E>
__device__ __forceinline__ void outbox_tile(const OBArgs &a, uint64_t t, uint64_t tb,
                                            uint32_t lane, uint64_t (&cnt)[O_N]) {
  const auto [g0, n, o8, live, gid] = tile_at(a.G, a.goff, t, lane);
  const uint32_t sz = a.wide ? 2u : 1u, full = (1u << a.S) - 1u;
  // ---- 1. the masks: who sends what ----
  const uint32_t ms = ob_ld_mask(ob_mask_rsrc(a.sent, g0, n, sz), lane, a.wide) & full;
  const uint32_t mp = ob_ld_mask(ob_mask_rsrc(a.snap, g0, n, sz), lane, a.wide) & full;
  const uint32_t mb = ob_ld_mask(ob_mask_rsrc(a.hb_sent, g0, n, sz), lane, a.wide) & full;
  const uint32_t ma = ms & ~mp, mh = mb & ~(ms | mp);  // MsgSnap, then MsgApp, then MsgHeartbeat
  const uint32_t m = ma | mp | mh;
  const bool has = live && m != 0;
  const uint32_t u = wave_or(m);  // the tile's mask union (wave-uniform)
  // ---- 2. once per tile: term, the log, the snapshot, the heartbeat context ----
  const uint64_t term = bld64<kNT>(mk_rsrc(a.term + g0, n * 8), has ? o8 : kOOB);
  const bool need_a = ma != 0, need_s = mp != 0, need_h = mh != 0;
  const bool need_log = need_a || (need_s && !a.snap_term);
  uint64_t rf[RM], rt[RM];
#pragma unroll
  for (int r = 0; r < RM; r++) {
    rf[r] = 0;
    rt[r] = 0;
  }
  uint64_t li = 0, committed = 0;
  uint32_t nr = 0;
  if (__builtin_amdgcn_ballot_w64(need_log)) {
    const uint32_t l8 = need_log ? o8 : kOOB;
    li = bld64<kNT>(mk_rsrc(a.last_index + g0, n * 8), l8);
    committed = bld64<kNT>(mk_rsrc(a.committed + g0, n * 8), need_a ? o8 : kOOB);
    nr = bld8<kNT>(mk_rsrc(a.run_count + g0, n), need_log ? lane : kOOB);
    nr = nr < a.R ? nr : a.R;
#pragma unroll
    for (int r = 0; r < RM; r++)
      if (static_cast<uint32_t>(r) < a.R) {
        const uint64_t row = static_cast<uint64_t>(r) * a.stride + g0;
        rf[r] = bld64<kNT>(mk_rsrc(a.run_first + row, n * 8), l8);
        rt[r] = bld64<kNT>(mk_rsrc(a.run_term + row, n * 8), l8);
      }
  }
  uint64_t sidx = 0, sterm = 0;
  if (__builtin_amdgcn_ballot_w64(need_s)) {
    const uint32_t s8 = need_s ? o8 : kOOB;
    sidx = bld64<kNT>(opt_rsrc(a.snap_src, g0, n), s8) - a.snap_sub;
    sterm = a.snap_term ? bld64<kNT>(mk_rsrc(a.snap_term + g0, n * 8), s8)
                        : run_term_at<RM>(rf, rt, nr, li, sidx);
  }
  uint32_t hctx = 0;
  if (__builtin_amdgcn_ballot_w64(need_h))
    hctx = bld32<kNT>(opt_rsrc(a.hb_ctx, g0, n), need_h ? lane * 4 : kOOB);
  // ---- 3. the per-slot rows of every slot in the union: m.Index of a MsgApp,
  // Commit of a MsgHeartbeat ----
  uint64_t v[QE_MAX_SLOTS];
#pragma unroll
  for (int s = 0; s < QE_MAX_SLOTS; s++) {
    v[s] = 0;
    if ((u >> s) & 1u) {
      const uint64_t row = static_cast<uint64_t>(s) * a.stride + g0;
      const bool ab = (ma >> s) & 1u, hb = (mh >> s) & 1u;
      uint64_t x = 0;
      if (a.index) {
        x = bld64<kNT>(mk_rsrc(a.index + row, n * 8), ab ? o8 : kOOB);
      } else if (a.next_before && __builtin_amdgcn_ballot_w64(ab)) {
        // Next - 1: from before the call where the peer replicates now
        const uint32_t pw = bld32<kNT>(mk_rsrc(a.peer + row, n * 4), ab ? lane * 4 : kOOB);
        const bool repl = (pw & QE_PF_STATE) == QE_PR_REPLICATE;
        x = (bld64<kNT>(mk_rsrc(a.next_before + row, n * 8), (ab && repl) ? o8 : kOOB) |
             bld64<kNT>(mk_rsrc(a.next + row, n * 8), (ab && !repl) ? o8 : kOOB)) -
            1u;
      }
      const uint64_t y = bld64<kNT>(opt_rsrc(a.hb_commit, row, n), hb ? o8 : kOOB);
      v[s] = ab ? x : y;
    }
  }
  // ---- 4. the records, slot by slot ----
  // what of the arrays this tile may write: capacity is the descriptors'
  const uint64_t tbc = tb < a.cap ? tb : a.cap;
  const uint32_t rem = static_cast<uint32_t>(a.cap - tbc < kObTileMax ? a.cap - tbc : kObTileMax);
  const rsrc_t d_group = mk_rsrc(a.o_group + tbc, rem * 8), d_to = mk_rsrc(a.o_to + tbc, rem),
               d_type = mk_rsrc(a.o_type + tbc, rem), d_term = mk_rsrc(a.o_term + tbc, rem * 8),
               d_index = mk_rsrc(a.o_index + tbc, rem * 8),
               d_lterm = mk_rsrc(a.o_log_term + tbc, rem * 8),
               d_commit = mk_rsrc(a.o_commit + tbc, rem * 8),
               d_ctx = a.o_ctx ? mk_rsrc(a.o_ctx + tbc, rem * 4) : mk_rsrc(a.o_ctx, 0);
  const uint64_t lim = a.max_entries ? a.max_entries : 0xFFFFFFFFull;
  uint32_t pbase = 0;
#pragma unroll
  for (int s = 0; s < QE_MAX_SLOTS; s++) {
    if (!((u >> s) & 1u)) continue;
    const bool bit = (m >> s) & 1u;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
    const uint32_t pos = pbase + lane_rank(bal);
    pbase += static_cast<uint32_t>(__builtin_popcountll(bal));
    const bool is_s = (mp >> s) & 1u, is_a = (ma >> s) & 1u, is_h = (mh >> s) & 1u;
    // MsgApp: LogTerm and the entries (i, hi] cut into the table's runs
    const uint64_t i = v[s];
    const bool bad = is_a && (nr == 0 || i < rf[0] || i > li);
    const bool app = is_a && !bad;
    const uint64_t hi = li - i > lim ? i + lim : li;
    uint32_t el[E > 0 ? E : 1] = {};
    uint64_t et[E > 0 ? E : 1] = {};
    uint32_t j = 0, ents = 0;
    if constexpr (E > 0) {
#pragma unroll
      for (int r = 0; r < RM; r++) {
        const uint64_t end = (r + 1 < RM && static_cast<uint32_t>(r + 1) < nr) ? rf[r + 1] - 1 : li;
        const uint64_t lo = rf[r] > i ? rf[r] : i + 1, e = end < hi ? end : hi;
        const bool ne = app && static_cast<uint32_t>(r) < nr && i < hi && lo <= e;
        const uint32_t len = static_cast<uint32_t>(e) - static_cast<uint32_t>(lo) + 1u;
#pragma unroll
        for (int k = 0; k < E; k++) {
          const bool sel = ne && j == static_cast<uint32_t>(k);
          el[k] = sel ? len : el[k];
          et[k] = sel ? rt[r] : et[k];
        }
        ents += (ne && j < static_cast<uint32_t>(E)) ? len : 0u;
        j += ne ? 1u : 0u;
      }
    }
    const uint32_t type =
        is_s ? QE_OMSG_SNAP : (bad ? QE_OMSG_BAD : (is_a ? QE_OMSG_APP : QE_OMSG_HEARTBEAT));
    const uint64_t idx = is_s ? sidx : (is_a ? i : 0);
    const uint64_t lt = is_s ? sterm : (app ? run_term_at<RM>(rf, rt, nr, li, i) : 0);
    const uint64_t cm = app ? committed : (is_h ? v[s] : 0);
    const uint32_t cx = is_h ? hctx : 0u;
    const uint32_t p1 = bit ? pos : kOOB, p4 = bit ? pos * 4 : kOOB, p8 = bit ? pos * 8 : kOOB;
    bst64<kNT>(gid, d_group, p8);
    bst8<kNT>(static_cast<uint32_t>(s), d_to, p1);
    bst8<kNT>(type, d_type, p1);
    bst64<kNT>(term, d_term, p8);
    bst64<kNT>(idx, d_index, p8);
    bst64<kNT>(lt, d_lterm, p8);
    bst64<kNT>(cm, d_commit, p8);
    bst32<kNT>(cx, d_ctx, p4);
    if constexpr (E > 0) {
#pragma unroll
      for (int k = 0; k < E; k++) {
        const uint64_t row = static_cast<uint64_t>(k) * a.cap + tbc;
        bst32<kNT>(el[k], mk_rsrc(a.o_ent_len + row, rem * 4), p4);
        bst64<kNT>(et[k], mk_rsrc(a.o_ent_term + row, rem * 8), p8);
      }
    }
    if (a.stats) {
      uint64_t h = mix64((gid * kPhi) ^ kOutboxSalt ^ (static_cast<uint64_t>(type) << 56) ^
                         (static_cast<uint64_t>(s) << 48));
      h = mix64(h ^ idx);
      h = mix64(h ^ lt);
      h = mix64(h ^ cm);
      h = mix64(h ^ ents);
      cnt[O_APP] += app ? 1u : 0u;
      cnt[O_SNAP] += is_s ? 1u : 0u;
      cnt[O_HB] += is_h ? 1u : 0u;
      cnt[O_BAD] += bad ? 1u : 0u;
      cnt[O_VIOL] += bad ? 1u : 0u;
      cnt[O_ENTRIES] += ents;
      cnt[O_CSUM] += bit ? h : 0u;
    }
  }
  cnt[O_GROUPS] += has ? 1u : 0u;
}

// A block per chunk (the blocks walk when the grid is capped for the
// statistics): the chunk's tile counts, their exclusive scan in every wave, then
// wave w fills the tiles 4k + w.
template <int RM, int E>
__global__ __launch_bounds__(kBlock) void k_outbox_fill(OBArgs a) {
  __shared__ uint32_t tcnt[kObTiles];
  uint64_t cnt[O_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t c = blockIdx.x; c < a.nb; c += gridDim.x) {
    chunk_tile_counts(a, a.wide != 0, c, tcnt);
    __syncthreads();
    const uint32_t x = tcnt[lane];
    __syncthreads();  // (the next chunk's counts overwrite tcnt)
    uint32_t inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d, 64);
      if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    const uint32_t pre = inc - x;
    const uint64_t cbase = a.offsets[c];
    for (uint32_t k = 0; k < kObRounds; k++) {
      const uint32_t T = k * (kBlock / 64) + w;
      if (__builtin_amdgcn_readfirstlane(__shfl(x, T, 64)) == 0) continue;  // no record
      const uint64_t tb = cbase + __builtin_amdgcn_readfirstlane(__shfl(pre, T, 64));
      outbox_tile<RM, E>(a, c * kObTiles + T, tb, lane, cnt);
    }
  }
  if (a.stats) {
    const int idx[O_N] = {QE_STAT_GROUPS,         QE_STAT_OUTBOX_APP,
                          QE_STAT_OUTBOX_SNAP,    QE_STAT_OUTBOX_HEARTBEAT,
                          QE_STAT_OUTBOX_BAD,     QE_STAT_INVARIANT_VIOLATIONS,
                          QE_STAT_OUTBOX_ENTRIES, QE_STAT_CHECKSUM};
    wave_stats_add<O_N>(cnt, idx, a.stats);
  }
}

}  // namespace qe
