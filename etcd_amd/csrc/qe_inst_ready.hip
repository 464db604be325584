// qe_inst_ready.hip — the Ready kernels' instantiations (qe_ready.hpp):
// k_ready_note, k_ready_count, k_advance, and k_ready_fill per run-capacity
// bucket (log_runs <= 4, <= 8, <= 16) and per run capacity of the lists
// (ent_runs 0..QE_MAX_MSG_RUNS).  None depends on the slot count at compile
// time, so this object is compiled once, not per QE_S.
#include "qe_ready.hpp"

namespace qe {

// One wave per chunk, four chunks per block, no block barrier.
__global__ __launch_bounds__(kBlock) void k_ready_count(RDArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t c =
      static_cast<uint64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= a.nb) return;  // (wave-uniform)
  const uint64_t base = c * kListChunk;
  const uint32_t nc = static_cast<uint32_t>(a.G - base < kListChunk ? a.G - base : kListChunk);
  const rsrc_t r_term = mk_rsrc(a.term + base, nc * 8), r_com = mk_rsrc(a.committed + base, nc * 8),
               r_li = mk_rsrc(a.last_index + base, nc * 8), r_rf = mk_rsrc(a.run_first + base, nc * 8),
               r_stb = mk_rsrc(a.stable + base, nc * 8), r_app = mk_rsrc(a.applied + base, nc * 8),
               r_snp = mk_rsrc(a.snap_pending + base, nc * 8),
               r_pt = mk_rsrc(a.prev_term + base, nc * 8),
               r_pc = mk_rsrc(a.prev_commit + base, nc * 8);
  const rsrc_t r_vote = opt_rsrc(a.vote, base, nc), r_lead = mk_rsrc(a.lead + base, nc),
               r_state = mk_rsrc(a.state + base, nc), r_pv = mk_rsrc(a.prev_vote + base, nc),
               r_pl = mk_rsrc(a.prev_lead + base, nc), r_ps = mk_rsrc(a.prev_state + base, nc),
               r_pend = opt_rsrc(a.pending, base, nc), r_flag = mk_rsrc(a.flag + base, nc);
  const uint32_t novote = a.vote ? 0u : 0xFFu;  // a NULL vote row: None
  uint32_t cnt = 0;
  if (a.vec && nc == kListChunk) {
#pragma unroll 2
    for (uint32_t j = 0; j < kListChunk / 128; j++) {
      const uint32_t q = j * 64 + lane;  // the pair of groups 2q, 2q + 1
      const u32x4 term = bld128(r_term, q * 16), com = bld128(r_com, q * 16),
                  li = bld128(r_li, q * 16), rf = bld128(r_rf, q * 16),
                  stb = bld128(r_stb, q * 16), app = bld128(r_app, q * 16),
                  snp = bld128(r_snp, q * 16), pt = bld128(r_pt, q * 16),
                  pc = bld128(r_pc, q * 16);
      const uint32_t vote = bld16(r_vote, q * 2) | novote | (novote << 8),
                     lead = bld16(r_lead, q * 2), state = bld16(r_state, q * 2),
                     pv = bld16(r_pv, q * 2), pl = bld16(r_pl, q * 2), ps = bld16(r_ps, q * 2),
                     pend = bld16(r_pend, q * 2);
      uint32_t f2 = 0;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const auto u64 = [h](u32x4 v) {
          return h ? (static_cast<uint64_t>(v.w) << 32 | v.z) : (static_cast<uint64_t>(v.y) << 32 | v.x);
        };
        const auto u8 = [h](uint32_t v) { return (v >> (8 * h)) & 0xFFu; };
        const uint32_t f = rd_flags(a.S, u64(term), u8(vote), u64(com), u8(lead), u8(state), u64(stb),
                                    u64(li), u64(app), u64(rf), u64(snp), u64(pt), u64(pc), u8(pv),
                                    u8(pl), u8(ps), u8(pend));
        const uint32_t on = (f & kRdListed) ? 1u : 0u;
        f2 |= on << (8 * h);
        cnt += on;
      }
      bst16(f2, r_flag, q * 2);
    }
  } else {
    for (uint32_t j = 0; j < kListChunk / 64; j++) {
      const uint32_t i = j * 64 + lane, o8 = i * 8;  // past nc: out of range, reads 0
      if (__builtin_amdgcn_readfirstlane(j * 64) >= nc) break;
      const uint32_t f = rd_flags(
          a.S, bld64(r_term, o8), bld8(r_vote, i) | novote, bld64(r_com, o8), bld8(r_lead, i),
          bld8(r_state, i), bld64(r_stb, o8), bld64(r_li, o8), bld64(r_app, o8), bld64(r_rf, o8),
          bld64(r_snp, o8), bld64(r_pt, o8), bld64(r_pc, o8), bld8(r_pv, i), bld8(r_pl, i),
          bld8(r_ps, i), bld8(r_pend, i));
      const uint32_t on = (i < nc && (f & kRdListed)) ? 1u : 0u;
      bst8(on, r_flag, i);
      cnt += on;
    }
  }
  cnt = wave_sum_u32(cnt);
  if (lane == 0) a.counts[c] = cnt;
}

// qe_ready_note: unstable.truncateAndAppend's `after <= offset` arm and
// unstable.restore (raft/log_unstable.go:115-141), a thread per group.
__global__ __launch_bounds__(kBlock) void k_ready_note(RNArgs a) {
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g < a.G;
       g += static_cast<uint64_t>(gridDim.x) * kBlock) {
    if (a.follow_result && a.follow_result[g] == QE_FR_APP_ACCEPT) {
      const uint64_t af = a.append_from[g];
      if (af != 0 && af - 1 < a.stable[g]) a.stable[g] = af - 1;
    }
    if (a.snap_result && a.snap_result[g] == QE_SR_RESTORED) {
      const uint64_t i = a.resp_index[g];
      a.stable[g] = i;
      a.snap_pending[g] = i;
    }
  }
}

// raftLog.term over the group's rows in memory (run_term_at of qe_step.hpp
// for a thread that holds one record, not a tile).
__device__ __forceinline__ uint64_t ad_term(const ADArgs &a, uint64_t g, uint64_t i) {
  uint32_t nr = a.run_count[g];
  nr = nr < a.R ? nr : a.R;
  if (nr == 0 || i < a.run_first[g] || i > a.last_index[g]) return 0;
  uint64_t t = 0;
  for (uint32_t r = 0; r < nr; r++) {
    const uint64_t k = static_cast<uint64_t>(r) * a.stride + g;
    t = i >= a.run_first[k] ? a.run_term[k] : t;
  }
  return t;
}

// qe_advance: acceptReady + RawNode.Advance + raft.advance, a thread per record.
__global__ __launch_bounds__(kBlock) void k_advance(ADArgs a) {
  const uint64_t c = *a.count, n = c < a.cap ? c : a.cap;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t g = a.group[i] - a.goff;
    if (g >= a.G) {
      a.result[i] = QE_ADV_BAD_GROUP;
      continue;
    }
    const uint32_t flags = a.flags[i];
    const uint64_t ac = a.apply_count[i];
    const uint64_t na = ac ? a.apply_first[i] + ac - 1 : ((flags & QE_RD_SNAP) ? a.snap_index[i] : 0);
    const uint64_t old = a.applied[g];
    if (na > 0 && (a.committed[g] < na || na < old)) {
      a.result[i] = QE_ADV_APPLIED_RANGE;
      continue;
    }
    uint32_t res = QE_ADV_OK;
    if (na > 0) a.applied[g] = na;
    if (flags & QE_RD_HARD) {
      a.prev_term[g] = a.term[i];
      a.prev_commit[g] = a.commit[i];
      a.prev_vote[g] = a.vote[i];
    }
    if (flags & QE_RD_SOFT) {
      a.prev_lead[g] = a.lead[i];
      a.prev_state[g] = a.state[i];
    }
    const uint64_t ec = a.ent_count[i];
    if (ec) {
      const uint64_t e = a.ent_first[i] + ec - 1;
      if (a.stable[g] < e && e <= a.last_index[g] && ad_term(a, g, e) == a.ent_last_term[i])
        a.stable[g] = e;
      else
        res = QE_ADV_OK_STALE_ENTRIES;
    }
    if ((flags & QE_RD_SNAP) && a.snap_pending[g] == a.snap_index[i]) a.snap_pending[g] = 0;
    if (na > 0 && a.auto_leave && a.auto_leave[g] && a.cur_state[g] == QE_STATE_LEADER) {
      const uint64_t pci = a.pending_conf_index[g];
      if (old <= pci && pci <= na) res |= QE_ADV_AUTO_LEAVE;
    }
    a.result[i] = static_cast<uint8_t>(res);
  }
}

int dispatch_ready_note(const RNArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_ready_note, dim3(elem_grid(a.G, num_cus())), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

// One wave per chunk; qe_ready has checked that the chunks fit a launch.
int dispatch_ready_count(const RDArgs &a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((a.nb + (kBlock / 64) - 1) / (kBlock / 64)));
  hipLaunchKernelGGL(k_ready_count, grid, dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

int dispatch_ready_fill(const RDArgs &a, uint32_t ent_runs, hipStream_t st) {
  const dim3 grid(list_fill_grid(a.nb, num_cus(), a.stats != nullptr));
  return with_run_bucket(a.R, [&](auto rm) {
    return with_msg_runs(ent_runs, [&](auto e) {
      hipLaunchKernelGGL((k_ready_fill<rm(), e()>), grid, dim3(kBlock), 0, st, a);
      return hip_status(hipGetLastError());
    });
  });
}

// The count is on the device: the grid covers the capacity and a thread past
// the count leaves at once.
int dispatch_advance(const ADArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_advance, dim3(elem_grid(a.cap, num_cus())), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
