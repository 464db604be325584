// qe_inst_applyconf.hip — the kernels of qe_apply_conf (qe_applyconf.hpp):
// k_apply_conf per slot count, and the two that are no templates, the clear of
// the scratch's `switched` row and the gather of the switch results.
#define QE_APPLYCONF_KERNELS
#include "qe_applyconf.hpp"

namespace qe {

// The `switched` row, 16 B per lane and store (qe_apply_conf pads the row to a
// multiple of 16 B on a 16-B boundary).
__global__ __launch_bounds__(kBlock) void k_apply_conf_clear(uint8_t *row, uint64_t bytes) {
  const uint64_t nq = bytes / 16;
  const u32x4 zero = {0, 0, 0, 0};
  for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kBlock; c < nq;
       c += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t left = nq - c;
    const uint32_t cnt = left < kBlock ? static_cast<uint32_t>(left) : kBlock;
    bst128(zero, mk_rsrc(row + c * 16, cnt * 16), threadIdx.x * 16);
  }
}

// sw_result of the records a leader applied: the switch kernel's byte of the
// record's group.  Every other record keeps the QE_SW_NONE k_apply_conf wrote.
__global__ __launch_bounds__(kBlock) void k_apply_conf_gather(ACArgs a) {
  const uint64_t n = ac_records(a);
  uint32_t lane;
  uint64_t wave, nwaves, ntiles;
  tile_walk(n, lane, wave, nwaves, ntiles);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const uint64_t r0 = t * 64;
    const uint32_t cnt = tile_n(n, t);
    const bool led = bld8<kNT>(mk_rsrc(a.result + r0, cnt), lane) == QE_AC_LEADER;
    if (!__builtin_amdgcn_ballot_w64(led)) continue;
    const uint64_t gid = bld64<kNT>(mk_rsrc(a.group + r0, cnt * 8), led ? lane * 8 : kOOB);
    // (a QE_AC_LEADER record's group is in the batch)
    const uint32_t sw = led ? a.swres[gid - a.goff] : 0u;
    bst8<kNT>(sw, mk_rsrc(a.sw_result + r0, cnt), led ? lane : kOOB);
  }
}

int dispatch_apply_conf_clear(uint8_t *row, uint64_t bytes, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_conf_clear, dim3(elem_grid(bytes / 16, num_cus())), dim3(kBlock), 0,
                     st, row, bytes);
  return hip_status(hipGetLastError());
}

// With the count on the device the grid covers the capacity and a wave past
// the count leaves at once.
static uint32_t apply_conf_grid(const ACArgs &a) {
  return tile_grid(a.count ? a.cap : a.n, num_cus(), false);
}

int dispatch_apply_conf(const ACArgs &a, uint32_t S, hipStream_t st) {
  return with_slots(S, [&](auto s) {
    hipLaunchKernelGGL(k_apply_conf<s()>, dim3(apply_conf_grid(a)), dim3(kBlock), 0, st, a);
    return hip_status(hipGetLastError());
  });
}

int dispatch_apply_conf_gather(const ACArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_conf_gather, dim3(apply_conf_grid(a)), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace qe
