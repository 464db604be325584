// qe_list.hpp — the record-list layer under qe_outbox, qe_replies, qe_ready and
// qe_read_states: what a call that turns per-group rows into a dense, ordered
// list of records shares with the others.  The routing layer (qe_route.hpp)
// uses it with a record of a list as the element in place of a group.
//
// Three passes over 4096-group chunks (64 tiles, a block of four waves each):
//   count   the records of each chunk (list_count_block; qe_ready has a count
//           pass of its own, which also writes the flags its fill reads);
//   scan    k_collect_scan (qe_collect.hpp, launched by the call): the chunk
//           offsets and the total;
//   fill    list_fill_walk: a block recounts its chunk's tiles (64 words of
//           LDS, the only LDS here), every wave scans them, and wave w writes
//           the tiles 4k + w that hold a record.  No block waits for another.
// A call brings two things.  Its counts: a functor that gives a thread the
// record counts of its 16 groups of a chunk, from bytes alone.  Its tile: a
// function in the house idiom (qe_step.hpp) that loads what the records of one
// 64-group tile need and stores them from position tb on, the records of a
// (kind, slot) at consecutive positions in lane order (ballot + lane_rank), so
// a wave's stores for one are one contiguous run; every store follows every
// load of the tile.  (qe_read_states is the exception to both: a group has a
// run of 0..257 records, so its tile scans the lanes' counts, a lane stores its
// own run from tb + its prefix on, and the book loads of one position of the
// runs follow the stores of the position before; qe_readstates.hpp.)  Capacity
// is the output descriptors' num_records (list_room): a record past it is an
// out-of-range store, dropped, with no branch.  Every access is non-temporal.
#pragma once
#include "qe_step.hpp"

namespace qe {

constexpr uint32_t kListRounds = 16;                     // groups per thread and chunk
constexpr uint32_t kListChunk = kBlock * kListRounds;    // groups per chunk (qe_collect's: qe_api.hip)
constexpr uint32_t kListTiles = kListChunk / 64;         // tiles per chunk
static_assert(kListTiles == 64, "a wave scans the tile counts of a chunk, one per lane");

// `cnt` elements of a mask-typed array from element `first` on (NULL: reads
// 0), and element i of it for the lanes with `on`.  The mask width is a
// run-time value here (mask_rsrc / ld_mask of qe_tile.hpp take it as a type).
__device__ __forceinline__ rsrc_t list_mask_rsrc(const void *p, uint64_t first, uint32_t cnt,
                                                 uint32_t sz) {
  return p ? mk_rsrc(static_cast<const uint8_t *>(p) + first * sz, cnt * sz) : mk_rsrc(p, 0);
}
__device__ __forceinline__ uint32_t list_ld_mask(rsrc_t r, uint32_t i, bool wide, bool on = true) {
  return wide ? bld16<kNT>(r, on ? i * 2 : kOOB) : bld8<kNT>(r, on ? i : kOOB);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
// The lane's rank among the lanes of a ballot.
__device__ __forceinline__ uint32_t lane_rank(uint64_t bal) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u));
}

// What of the record arrays a tile whose first record has position tb may
// write: `rem` records from tbc on (tile_max: the records of one tile at most).
struct ListRoom {
  uint64_t tbc;
  uint32_t rem;
};
__device__ __forceinline__ ListRoom list_room(uint64_t tb, uint64_t cap, uint32_t tile_max) {
  const uint64_t tbc = tb < cap ? tb : cap;
  return {tbc, static_cast<uint32_t>(cap - tbc < tile_max ? cap - tbc : tile_max)};
}

// The group of the chunk a thread takes in round r.
__device__ __forceinline__ uint32_t list_elem(uint32_t r) { return r * kBlock + threadIdx.x; }

// The records of each tile of chunk c into tcnt[kListTiles].  Thread t takes
// the chunk's groups list_elem(r), so round r of wave w is tile 4r + w.
// counts(base, nc, k) gives the thread their record counts k[r] from the rows
// of the chunk (nc groups from group `base` on); an element past nc is out of
// range and reads 0.
template <class F>
__device__ __forceinline__ void list_chunk_counts(uint64_t G, uint64_t c, uint32_t *tcnt,
                                                  const F &counts) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t base = c * kListChunk;
  const uint32_t nc = static_cast<uint32_t>(G - base < kListChunk ? G - base : kListChunk);
  uint32_t k[kListRounds];
  counts(base, nc, k);
#pragma unroll
  for (uint32_t r = 0; r < kListRounds; r++) {
    const uint32_t s = wave_sum_u32(k[r]);
    if (lane == 0) tcnt[r * (kBlock / 64) + w] = s;
  }
}

// The count kernel: one block per chunk.
template <class F>
__device__ __forceinline__ void list_count_block(uint64_t G, uint32_t *chunk_counts,
                                                 const F &counts) {
  __shared__ uint32_t tcnt[kListTiles];
  list_chunk_counts(G, blockIdx.x, tcnt, counts);
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t s = wave_sum_u32(tcnt[threadIdx.x]);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = s;
  }
}

// The fill kernel: a block per chunk (the blocks walk when the grid is capped
// for the statistics, list_fill_grid of qe_launch.hpp): the chunk's tile
// counts, their exclusive scan in every wave, then wave w fills the tiles
// 4k + w with Tile(a, t, tb, lane, cnt).  The wave's counters cnt[N] go to the
// statistics idx[N].  A: the call's arguments (G, nb, offsets, stats).
template <auto Tile, int N, class A, class F>
__device__ __forceinline__ void list_fill_walk(const A &a, const int (&idx)[N], const F &counts) {
  __shared__ uint32_t tcnt[kListTiles];
  uint64_t cnt[N] = {};
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t c = blockIdx.x; c < a.nb; c += gridDim.x) {
    list_chunk_counts(a.G, c, tcnt, counts);
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
    for (uint32_t k = 0; k < kListRounds; k++) {
      const uint32_t T = k * (kBlock / 64) + w;
      if (__builtin_amdgcn_readfirstlane(__shfl(x, T, 64)) == 0) continue;  // no record
      const uint64_t tb = cbase + __builtin_amdgcn_readfirstlane(__shfl(pre, T, 64));
      Tile(a, c * kListTiles + T, tb, lane, cnt);
    }
  }
  if (a.stats) wave_stats_add<N>(cnt, idx, a.stats);
}

}  // namespace qe
