// qe_route.hpp — the routing layer under qe_inbox and qe_requests: what a call
// that routes a list of records into per-group rows shares with the other.
//
// Each call restates a sequential per-group rule in an order-free form.  The
// key of record i is i + 1.  Per group there are scratch words, kRouteNone =
// nobody lowered it, each the result of 32-bit atomicMin (any arrival order
// gives the same minimum, so the outputs are bit-exact from run to run); one is
// stop[g], the lowest key that ends what the group takes in this pass.  A
// G-sized init pass resets the words and the complete type rows, key passes
// lower them, and a routing pass writes the dispositions, the rows and a
// deferred flag byte per record; the record-list layer (qe_list.hpp, a record
// as its element) turns the flags into the ascending deferred positions.
// One lane per record, one wave per 64-record tile: the SoA loads go through
// per-tile buffer descriptors (coalesced, the ragged last tile clipped).  A
// record's destination is any group of the batch, so the scatters, the gathers
// of the receiver's rows and the scratch words are addressed with 64-bit
// pointers under the lane's predicate (the bounds check: g - group_offset < G,
// from < S); a 32-bit descriptor offset would not span [S][stride] rows.
// Here: the head of a record, the checksum term, a flag array's counts and the
// positions fill.  A call brings its validity rule, words and passes.
#pragma once
#include "qe_list.hpp"

namespace qe {

constexpr uint32_t kRouteNone = 0xFFFFFFFFu;  // a scratch word nobody lowered

// The arguments of the positions fill: the layer's element is a record, so its
// G is the list's length.  `out` holds G positions: no capacity to enforce.
struct RoutePos {
  uint64_t G, nb;
  const uint64_t *offsets;  // k_collect_scan's, per 4096-record chunk
  const uint8_t *flag;      // [G]
  uint32_t *out;
  static constexpr uint64_t *stats = nullptr;  // the routing pass holds the statistics
};

// defined in qe_inst_route.hip
int dispatch_route_positions(const RoutePos &a, hipStream_t st);

// The kernels are defined in the objects that launch them, which set
// QE_ROUTE_KERNELS (qe_inst_route.hip, qe_inst_carry.hip); qe_api.hip takes the
// argument structs and the dispatchers.
#ifdef QE_ROUTE_KERNELS

// Record `lane` of tile t: its key, group (global and local), slot and type,
// and whether its group is in a batch of G (the bounds check of every access
// addressed by g).
struct RouteRec {
  uint32_t key, from, type;
  uint64_t gid, g;
  bool live;
};
__device__ __forceinline__ void route_rec(RouteRec &r, const uint64_t *group, const uint8_t *from,
                                          const uint8_t *type, uint64_t n, uint64_t goff,
                                          uint64_t t, uint32_t lane) {
  const uint64_t r0 = t * 64;
  const uint32_t cnt = tile_n(n, t);
  r.live = lane < cnt;
  r.key = static_cast<uint32_t>(r0) + lane + 1u;
  r.gid = bld64<kNT>(mk_rsrc(group + r0, cnt * 8), lane * 8);
  r.from = bld8<kNT>(mk_rsrc(from + r0, cnt), lane);
  r.type = bld8<kNT>(mk_rsrc(type + r0, cnt), lane);
  r.g = r.gid - goff;
}

// The record's term of QE_STAT_CHECKSUM (record_hashes of tests/inbox_model.py).
__device__ __forceinline__ uint64_t route_hash(uint64_t gid, uint64_t salt, uint32_t disp,
                                               uint32_t type, uint32_t from, uint32_t pos) {
  const uint64_t h = mix64((gid * kPhi) ^ salt ^ (static_cast<uint64_t>(disp) << 56) ^
                           (static_cast<uint64_t>(type) << 48) ^ (static_cast<uint64_t>(from) << 40));
  return mix64(h ^ pos);
}

// The counts of the layer: a record's flag byte.
struct FlagCounts {
  const uint8_t *flag;
  __device__ __forceinline__ void operator()(uint64_t base, uint32_t nc,
                                             uint32_t (&k)[kListRounds]) const {
    const rsrc_t rf = mk_rsrc(flag + base, nc);
#pragma unroll
    for (uint32_t r = 0; r < kListRounds; r++) k[r] = bld8<kNT>(rf, list_elem(r)) != 0 ? 1u : 0u;
  }
};

// Tile t of the list, whose first flagged record has position tb in `out`.
__device__ __forceinline__ void route_positions_tile(const RoutePos &a, uint64_t t, uint64_t tb,
                                                     uint32_t lane, uint64_t (&)[1]) {
  const uint64_t r0 = t * 64;
  const uint32_t n = tile_n(a.G, t);
  const bool has = bld8<kNT>(mk_rsrc(a.flag + r0, n), lane) != 0;
  const uint32_t pos = lane_rank(__builtin_amdgcn_ballot_w64(has));
  const auto [tbc, rem] = list_room(tb, a.G, 64);
  bst32<kNT>(static_cast<uint32_t>(r0) + lane, mk_rsrc(a.out + tbc, rem * 4),
             has ? pos * 4 : kOOB);
}

// The positions of the flagged records, ascending: defined in the one object
// that also sets QE_ROUTE_POSITIONS_KERNEL (qe_inst_route.hip).
#ifdef QE_ROUTE_POSITIONS_KERNEL
__global__ __launch_bounds__(kBlock) void k_route_positions(RoutePos a) {
  const int idx[1] = {QE_STAT_GROUPS};
  list_fill_walk<route_positions_tile>(a, idx, FlagCounts{a.flag});
}
#endif
#endif  // QE_ROUTE_KERNELS

}  // namespace qe
