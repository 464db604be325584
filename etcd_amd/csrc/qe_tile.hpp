// qe_tile.hpp — what every one-lane-per-group kernel uses: the cache policy
// of its accesses, the buffer loads and stores, the walk of a wave over its
// 64-group tiles, a tile's row of a mask-typed array, and the ReadIndex
// queue's pending context.  The Progress kernels (qe_progress.hpp) and the
// step kernels (qe_step.hpp and the headers on it) are built on it.
//
// Accesses go through per-tile buffer descriptors (wave-uniform base, 32-bit
// lane offset, num_records clipping the ragged last tile), as in the stream
// commit/vote kernel (qe_stream.hpp): a conditional access is an
// unconditional load or store whose offset is pushed out of range when its
// condition is false (no traffic, no branch, loads return 0).
#pragma once
#include "qe_stream.hpp"

namespace qe {

// Cache policy of the accesses (the helpers' AUX: 0 = default, 2 =
// non-temporal).  The Progress step re-touches the lines it loads
// (non-temporal loads: +15 %) and so does CheckQuorum (+17 %); the send
// kernel's appends and Progress rows go non-temporal, kNT: -9 %
// (profiles/r04/pstep_ab.txt, send_cq_nt_ab.txt), and so does every row a step
// kernel touches once per launch.
// QE_LD_AUX / QE_ST_AUX: A/B knobs for the default.
#ifndef QE_LD_AUX
#define QE_LD_AUX 0
#endif
#ifndef QE_ST_AUX
#define QE_ST_AUX 0
#endif
#ifndef QE_SEND_AUX  // A/B knob: the send kernel's policy
#define QE_SEND_AUX 2
#endif
constexpr int kNT = QE_SEND_AUX;
template <int AUX = QE_LD_AUX>
__device__ __forceinline__ uint64_t bld64(rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, AUX));
}
template <int AUX = QE_LD_AUX>
__device__ __forceinline__ uint32_t bld8(rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b8(r, off, 0, AUX);
}
template <int AUX = QE_ST_AUX>
__device__ __forceinline__ void bst64(uint64_t v, rsrc_t r, uint32_t off) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, off, 0, AUX);
}
template <int AUX = QE_ST_AUX>
__device__ __forceinline__ void bst8(uint32_t v, rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v), r, off, 0, AUX);
}
template <int AUX = QE_LD_AUX>
__device__ __forceinline__ uint32_t bld16(rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, AUX);
}
template <int AUX = QE_ST_AUX>
__device__ __forceinline__ void bst16(uint32_t v, rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(v), r, off, 0, AUX);
}
template <int AUX = QE_LD_AUX>
__device__ __forceinline__ uint32_t bld32(rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX);
}
template <int AUX = QE_ST_AUX>
__device__ __forceinline__ void bst32(uint32_t v, rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b32(v, r, off, 0, AUX);
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 bld128(rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, QE_LD_AUX));
}
__device__ __forceinline__ void bst128(u32x4 v, rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, QE_ST_AUX);
}

// A tile's row of a mask-typed array (MT = u8 for up to 8 slots, u16 above)
// for the lanes with `on`: no bytes move for the others.  The descriptor says
// what a NULL array means: mk_rsrc for a row that is there, mask_rsrc for an
// optional one (reads as 0, drops its stores).
template <typename MT>
__device__ __forceinline__ rsrc_t mask_rsrc(const void *p, uint64_t g0, uint32_t n) {
  return opt_rsrc(static_cast<const MT *>(p), g0, n);
}
template <typename MT, int AUX = 0>
__device__ __forceinline__ uint32_t ld_mask(rsrc_t r, uint32_t lane, bool on = true) {
  const uint32_t off = on ? lane * static_cast<uint32_t>(sizeof(MT)) : kOOB;
  if constexpr (sizeof(MT) == 1)
    return bld8<AUX>(r, off);
  else
    return bld16<AUX>(r, off);
}
template <typename MT, int AUX = 0>
__device__ __forceinline__ void bst_mask(uint32_t v, rsrc_t r, uint32_t lane, bool on = true) {
  const uint32_t off = on ? lane * static_cast<uint32_t>(sizeof(MT)) : kOOB;
  if constexpr (sizeof(MT) == 1)
    bst8<AUX>(v, r, off);
  else
    bst16<AUX>(v, r, off);
}
// A configuration mask (tracked, inc_mask, out_mask) clipped to the S slots.
template <typename MT, int S>
__device__ __forceinline__ uint32_t ld_slot_mask(const void *p, uint64_t g0, uint32_t n,
                                                 uint32_t lane, bool on = true) {
  return ld_mask<MT>(mk_rsrc(static_cast<const MT *>(p) + g0, n * sizeof(MT)), lane, on) &
         ((1u << S) - 1u);
}

// One lane per group, one wave per 64-group tile: the lane, the wave's first
// tile, the stride of its walk and the tile count.
__device__ __forceinline__ void tile_walk(uint64_t G, uint32_t &lane, uint64_t &wave,
                                          uint64_t &nwaves, uint64_t &ntiles) {
  lane = threadIdx.x & 63;
  wave = static_cast<uint64_t>(blockIdx.x) * (kBlock / 64) +
         __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  nwaves = static_cast<uint64_t>(gridDim.x) * (kBlock / 64);
  ntiles = (G + 63) / 64;
}

// The ReadIndex queue: the pending count (a count above the capacity is
// invalid input) and readOnly.lastPendingRequestCtx, the
// context of the newest pending request, 0 with none.
__device__ __forceinline__ uint32_t read_pending(uint32_t count, uint32_t cap) {
  return count < cap ? count : cap;
}
__device__ __forceinline__ uint32_t last_pending_ctx(uint32_t count, uint32_t head, uint32_t cap) {
  const uint32_t q = read_pending(count, cap);
  return q ? head + q - 1u : 0u;
}

// The checksum salt of a CheckQuorum (k_check_quorum) and of a tick, whose
// CheckQuorum it runs (k_tick): quorum active.
constexpr uint64_t kQuorumSalt = 0xA0761D6478BD642Full;

}  // namespace qe
