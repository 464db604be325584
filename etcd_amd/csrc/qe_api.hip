// qe_api.hip — C ABI of include/etcd_quorum.h: argument checks, alignment
// selection of the vectorised path and launch of the MI355X kernels.
#include <stdio.h>
#include <string.h>

#include "qe_dispatch.hpp"
#include "qe_conf.hpp"
#include "qe_collect.hpp"
#include "qe_tick.hpp"
#include "qe_follow.hpp"
#include "qe_vote.hpp"
#include "qe_snap.hpp"
#include "qe_outbox.hpp"
#include "qe_inbox.hpp"
#include "qe_replies.hpp"
#include "qe_ready.hpp"
#include "qe_readstates.hpp"
#include "qe_requests.hpp"
#include "qe_applyconf.hpp"
#include "qe_carry.hpp"

namespace qe {

int g_blocks_per_cu = 0;  // 0 = kernel occupancy
int g_nontemporal = 3;  // nt loads + nt stores (measured best)
int g_tiles_per_wave = -1;  // -1 = per-kernel default, 0 = persistent grid
int g_cv_kernel = -1;  // qe_commit_vote kernel: 0 pair, 1 stream, -1 per-mode default
int g_repl_kernel = -1;  // qe_replication_round kernel: 0 pair, 1 stream, -1 default

static thread_local char g_errbuf[256];

void set_error(const char *msg) { snprintf(g_errbuf, sizeof(g_errbuf), "%s", msg); }

int hip_status(hipError_t e) {
  if (e == hipSuccess) return QE_OK;
  snprintf(g_errbuf, sizeof(g_errbuf), "HIP error %d: %s", static_cast<int>(e),
           hipGetErrorString(e));
  return QE_EHIP;
}

static inline bool al(const void *p, size_t a) {
  return (reinterpret_cast<uintptr_t>(p) % a) == 0;
}

// Sparse MsgAppResp acks: Progress.MaybeUpdate with 64-bit atomic max.
__global__ __launch_bounds__(kBlock) void k_apply_acks(uint64_t G, uint32_t S, uint64_t stride,
                                                       uint64_t *match, uint64_t *next,
                                                       uint64_t n, const uint64_t *group,
                                                       const int8_t *slot,
                                                       const uint64_t *index,
                                                       uint8_t *touched) {
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint64_t g = group[i];
    const int s = slot[i];
    if (g >= G || s < 0 || s >= static_cast<int>(S)) continue;
    const uint64_t x = index[i];
    const uint64_t off = static_cast<uint64_t>(s) * stride + g;
    atomicMax(reinterpret_cast<unsigned long long *>(match + off),
              static_cast<unsigned long long>(x));
    if (x != ~0ull)  // next = max(next, x+1); x+1 wraps only for x = max
      atomicMax(reinterpret_cast<unsigned long long *>(next + off),
                static_cast<unsigned long long>(x + 1));
    if (touched) touched[g] = 1;
  }
}

__global__ void k_stats_reduce(const uint64_t *stats, uint64_t *out) {
  const int c = threadIdx.x;
  if (c < QE_STATS_COUNTERS) {
    uint64_t s = 0;
    for (int k = 0; k < QE_STATS_SHARDS; k++) s += stats[k * QE_STATS_COUNTERS + c];
    out[c] = s;
  }
}


}  // namespace qe

// ===========================================================================
// C ABI
// ===========================================================================
using namespace qe;

// The scratch part every list call shares with qe_collect: the chunk offsets
// (u64, so the scratch is 8-B aligned at the start), then the chunk counts (u32).
static_assert(kListChunk == kCollectChunk, "k_collect_count's and k_collect_scan's chunks");
struct ScanScratch {
  int status;  // QE_OK; QE_ERANGE when the chunks pass the 2^31 - 1 blocks of a launch
  uint64_t nb;  // chunks
  uint64_t *offsets;
  uint32_t *counts;
};
static uint64_t scan_chunks(uint64_t n) { return (n + kCollectChunk - 1) / kCollectChunk; }
static ScanScratch scan_scratch(void *scratch, uint64_t n) {
  const uint64_t nb = scan_chunks(n);
  if (nb > 0x7FFFFFFFull) return {QE_ERANGE, 0, nullptr, nullptr};
  uint64_t *offsets = static_cast<uint64_t *>(scratch);
  return {QE_OK, nb, offsets, reinterpret_cast<uint32_t *>(offsets + nb)};
}
// k_collect_count: the set flags of each chunk of flags[n].
static void launch_count(const uint8_t *flags, uint64_t n, const ScanScratch &sc, hipStream_t st) {
  hipLaunchKernelGGL(k_collect_count, dim3(static_cast<unsigned>((sc.nb + kCountWaves - 1) / kCountWaves)),
                     dim3(kBlock), 0, st, flags, n, al(flags, 16), sc.nb, sc.counts);
}
// k_collect_scan: the exclusive prefix of the chunk counts and the total.
static int launch_scan(const ScanScratch &sc, uint64_t *total, hipStream_t st) {
  hipLaunchKernelGGL(k_collect_scan, dim3(1), dim3(1024), 0, st, sc.counts, sc.nb, sc.offsets,
                     total);
  return hip_status(hipGetLastError());
}

// A cursor over a call's scratch: take<T>(k) is the next k elements of T.  Over
// NULL it only measures, so a call's qe_*_scratch_bytes and the pointers the
// call uses come from one routine.
struct Carve {
  void *base;
  size_t at = 0;
  template <class T>
  T *take(uint64_t k) {
    T *p = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + at);
    at += static_cast<size_t>(k * sizeof(T));
    return p;
  }
};

// qe_inbox's scratch for a.G, a.S and a.n into `a` and `sc` -> its size:
// qe_collect's part for n flags (offsets u64, counts u32, its 64 B of slack),
// the words first / stop / hi [G] and cell [S][G], the flags [n].
static size_t inbox_scratch(void *scratch, IBArgs &a, ScanScratch &sc) {
  Carve c{scratch};
  const uint64_t nb = scan_chunks(a.n);
  sc = {QE_OK, nb, c.take<uint64_t>(nb), c.take<uint32_t>(nb)};
  c.take<uint8_t>(64);
  a.first = c.take<uint32_t>(a.G);
  a.stop = c.take<uint32_t>(a.G);
  a.hi = c.take<uint32_t>(a.G);
  a.cell = c.take<uint32_t>(a.S * a.G);
  a.dflag = c.take<uint8_t>(a.n);
  return c.at;
}

// qe_requests's scratch for a.G and a.n into `a`, `sd` (the deferred list) and
// `so` (the output list) -> its size: the chunk offsets of both lists (u64),
// their chunk counts (u32), the words stop [G], the flags dflag and okind [n],
// qe_collect's 64 B of slack per list.
static size_t requests_scratch(void *scratch, RQArgs &a, ScanScratch &sd, ScanScratch &so) {
  Carve c{scratch};
  const uint64_t nb = scan_chunks(a.n);
  uint64_t *off = c.take<uint64_t>(2 * nb);
  uint32_t *cnt = c.take<uint32_t>(2 * nb);
  sd = {QE_OK, nb, off, cnt};
  so = {QE_OK, nb, off + nb, cnt + nb};
  a.stop = c.take<uint32_t>(a.G);
  a.dflag = c.take<uint8_t>(a.n);
  a.okind = c.take<uint8_t>(a.n);
  c.take<uint8_t>(2 * 64);
  return c.at;
}

// qe_carry's scratch for a.G (the source's capacity) into `a`, `sl` (the local
// list) and `sr` (the remote positions) -> its size: the chunk offsets of both
// lists (u64), their chunk counts (u32), the count and remote flag bytes [a.G],
// qe_collect's 64 B of slack per list.
static size_t carry_scratch(void *scratch, CRArgs &a, ScanScratch &sl, ScanScratch &sr) {
  Carve c{scratch};
  const uint64_t nb = scan_chunks(a.G);
  uint64_t *off = c.take<uint64_t>(2 * nb);
  uint32_t *cnt = c.take<uint32_t>(2 * nb);
  sl = {QE_OK, nb, off, cnt};
  sr = {QE_OK, nb, off + nb, cnt + nb};
  a.nb = nb;
  a.offsets = sl.offsets;
  a.counts = sl.counts;
  a.kcnt = c.take<uint8_t>(a.G);
  a.rflag = c.take<uint8_t>(a.G);
  c.take<uint8_t>(2 * 64);
  return c.at;
}

// The head the argument struct of every step kernel (qe_follower_step, qe_vote_step,
// qe_snapshot_step, qe_compact) starts with, and the statistics.
template <class A>
static void step_head(const qe_progress *p, uint64_t *stats, A &a) {
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.R = p->log_runs;
  a.stats = stats;
}

extern "C" {

int qe_abi_version(void) { return QE_ABI_VERSION; }

const char *qe_strerror(int status) {
  switch (status) {
    case QE_OK: return "ok";
    case QE_EINVAL: return "invalid argument";
    case QE_ERANGE: return "out of range";
    case QE_EHIP: return g_errbuf[0] ? g_errbuf : "HIP error";
    case QE_ECOMM: return g_errbuf[0] ? g_errbuf : "RCCL error";
    default: return "unknown status";
  }
}

size_t qe_mask_bytes(uint32_t num_slots) {
  if (num_slots == 0 || num_slots > QE_MAX_SLOTS) return 0;
  return num_slots <= 8 ? 1 : 2;
}

// Optional tuning knobs (not part of the reference semantics):
//   "blocks_per_cu"  cap on persistent-grid workgroups per CU (0 = occupancy)
//   "tiles_per_wave" -1 = per-kernel default, 0 = persistent grid,
//                    T > 0 = each wave walks T tiles
//   "nontemporal"    bit 0: non-temporal loads, bit 1: non-temporal stores
//   "cv_kernel", "repl_kernel"  0 = pair kernel, 1 = stream kernel, -1 = default
int qe_tune(const char *key, int value) {
  if (!key) return QE_EINVAL;
  if (!strcmp(key, "blocks_per_cu")) {
    if (value < 0 || value > 32) return QE_ERANGE;
    g_blocks_per_cu = value;
    return QE_OK;
  }
  if (!strcmp(key, "tiles_per_wave")) {
    if (value < -1 || value > 4096) return QE_ERANGE;
    g_tiles_per_wave = value;
    return QE_OK;
  }
  if (!strcmp(key, "cv_kernel")) {
    if (value < -1 || value > 1) return QE_ERANGE;
    g_cv_kernel = value;
    return QE_OK;
  }
  if (!strcmp(key, "repl_kernel")) {
    if (value < -1 || value > 1) return QE_ERANGE;
    g_repl_kernel = value;
    return QE_OK;
  }
  if (!strcmp(key, "nontemporal")) {
    if (value < 0 || value > 3) return QE_ERANGE;
    g_nontemporal = value;
    return QE_OK;
  }
  return QE_EINVAL;
}

static int check_groups(const qe_groups *g) {
  if (!g) return QE_EINVAL;
  if (g->num_slots == 0 || g->num_slots > QE_MAX_SLOTS) return QE_EINVAL;
  if (g->reserved != 0) return QE_EINVAL;
  if (g->num_groups && g->stride < g->num_groups) return QE_EINVAL;
  if (g->out_mask && !g->inc_mask) return QE_EINVAL;
  return QE_OK;
}

int qe_commit_vote(const qe_groups *g, const qe_outputs *out, void *stream) {
  int rc = check_groups(g);
  if (rc) return rc;
  if (!out) return QE_EINVAL;
  if (g->num_groups == 0) return QE_OK;
  if (!g->match) return QE_EINVAL;
  CVArgs a{};
  a.G = g->num_groups;
  a.goff = g->group_offset;
  a.stride = g->stride;
  a.match = g->match;
  a.inc = g->inc_mask;
  a.out = g->out_mask;
  a.learner = g->learner_mask;
  a.voted = g->voted;
  a.granted = g->granted;
  a.commit = out->commit;
  a.vote = out->vote;
  a.gcount = out->granted_count;
  a.rcount = out->rejected_count;
  a.stats = out->stats;
  const int mode = g->out_mask ? 2 : (g->inc_mask ? 1 : 0);
  const size_t mb = qe_mask_bytes(g->num_slots);
  bool vec = al(g->match, 16) && (g->stride % 2 == 0) && al(out->commit, 16);
  const void *masks[] = {g->inc_mask, g->out_mask, g->learner_mask, g->voted, g->granted};
  for (const void *m : masks) vec = vec && al(m, 2 * mb);
  const uint8_t *bytes[] = {out->vote, out->granted_count, out->rejected_count};
  for (const uint8_t *b : bytes) vec = vec && al(b, 2);
  return with_slots(g->num_slots, [&](auto s) {
    return dispatch_cv<s()>(a, mode, vec, static_cast<hipStream_t>(stream));
  });
}

int qe_committed_index(const qe_groups *g, uint64_t *commit, void *stream) {
  if (!g || !commit) return QE_EINVAL;
  qe_groups gg = *g;
  gg.voted = nullptr;
  gg.granted = nullptr;
  qe_outputs o{};
  o.commit = commit;
  return qe_commit_vote(&gg, &o, stream);
}

int qe_vote_result(const qe_groups *g, uint8_t *vote, void *stream) {
  int rc = check_groups(g);
  if (rc) return rc;
  if (!vote) return QE_EINVAL;
  if (g->num_groups == 0) return QE_OK;
  const uint32_t full = (1u << g->num_slots) - 1u;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = elem_grid(g->num_groups, num_cus());
  if (g->num_slots <= 8)
    hipLaunchKernelGGL(k_vote_result<uint8_t>, dim3(grid), dim3(kBlock), 0, st, g->num_groups,
                       full, g->inc_mask, g->out_mask, g->voted, g->granted, vote);
  else
    hipLaunchKernelGGL(k_vote_result<uint16_t>, dim3(grid), dim3(kBlock), 0, st,
                       g->num_groups, full, g->inc_mask, g->out_mask, g->voted, g->granted,
                       vote);
  return hip_status(hipGetLastError());
}

int qe_quorum_active(const qe_groups *g, const void *recent_active, uint8_t *active,
                     void *stream) {
  int rc = check_groups(g);
  if (rc) return rc;
  if (!recent_active || !active) return QE_EINVAL;
  if (g->num_groups == 0) return QE_OK;
  const uint32_t full = (1u << g->num_slots) - 1u;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = elem_grid(g->num_groups, num_cus());
  if (g->num_slots <= 8)
    hipLaunchKernelGGL(k_quorum_active<uint8_t>, dim3(grid), dim3(kBlock), 0, st,
                       g->num_groups, full, g->inc_mask, g->out_mask, g->learner_mask,
                       recent_active, active);
  else
    hipLaunchKernelGGL(k_quorum_active<uint16_t>, dim3(grid), dim3(kBlock), 0, st,
                       g->num_groups, full, g->inc_mask, g->out_mask, g->learner_mask,
                       recent_active, active);
  return hip_status(hipGetLastError());
}

int qe_record_votes(uint64_t num_groups, uint32_t num_slots, void *voted, void *granted,
                    const void *resp_mask, const void *resp_value, void *stream) {
  if (num_slots == 0 || num_slots > QE_MAX_SLOTS) return QE_EINVAL;
  if (num_groups == 0) return QE_OK;
  if (!voted || !granted || !resp_mask || !resp_value) return QE_EINVAL;
  const uint32_t full = (1u << num_slots) - 1u;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = elem_grid(num_groups, num_cus());
  if (num_slots <= 8)
    hipLaunchKernelGGL(k_record_votes<uint8_t>, dim3(grid), dim3(kBlock), 0, st, num_groups,
                       full, voted, granted, resp_mask, resp_value);
  else
    hipLaunchKernelGGL(k_record_votes<uint16_t>, dim3(grid), dim3(kBlock), 0, st, num_groups,
                       full, voted, granted, resp_mask, resp_value);
  return hip_status(hipGetLastError());
}

int qe_replication_round(const qe_repl_state *s, const qe_repl_msgs *m, uint64_t *stats,
                         void *stream) {
  if (!s || !m) return QE_EINVAL;
  if (s->num_slots == 0 || s->num_slots > QE_MAX_SLOTS || s->reserved) return QE_EINVAL;
  if (s->num_groups == 0) return QE_OK;
  if (s->stride < s->num_groups) return QE_EINVAL;
  if (!s->match || !s->next || !s->committed || !s->term_start || !s->last_index ||
      !m->resp_index)
    return QE_EINVAL;
  if (s->out_mask && !s->inc_mask) return QE_EINVAL;
  RArgs a{};
  a.G = s->num_groups;
  a.goff = s->group_offset;
  a.stride = s->stride;
  a.match = s->match;
  a.next = s->next;
  a.committed = s->committed;
  a.term_start = s->term_start;
  a.last_index = s->last_index;
  a.resp = m->resp_index;
  a.inc = s->inc_mask;
  a.out = s->out_mask;
  a.resp_mask = m->resp_mask;
  a.read_acks = m->read_acks;
  a.read_ok = m->read_ok;
  a.adv = m->commit_advanced;
  a.stats = stats;
  const size_t mb = qe_mask_bytes(s->num_slots);
  bool vec = (s->stride % 2 == 0);
  const void *p16[] = {s->match, s->next, s->committed, s->term_start, s->last_index,
                       m->resp_index};
  for (const void *p : p16) vec = vec && al(p, 16);
  const void *pm[] = {s->inc_mask, s->out_mask, m->resp_mask, m->read_acks};
  for (const void *p : pm) vec = vec && al(p, 2 * mb);
  vec = vec && al(m->read_ok, 2) && al(m->commit_advanced, 2);
  return with_slots(s->num_slots, [&](auto n) {
    return dispatch_repl<n()>(a, s->inc_mask != nullptr, s->out_mask != nullptr, vec,
                              static_cast<hipStream_t>(stream));
  });
}

int qe_election_steps(const qe_election_state *s, const qe_election_params *p, uint64_t *stats,
                      void *stream) {
  if (!s || !p) return QE_EINVAL;
  if (s->num_slots == 0 || s->num_slots > QE_MAX_SLOTS || s->reserved) return QE_EINVAL;
  if (s->num_groups == 0) return QE_OK;
  if (!s->term || !s->state || !s->voted || !s->granted || !s->self_slot) return QE_EINVAL;
  if (s->out_mask && !s->inc_mask) return QE_EINVAL;
  if (p->p_drop_q16 > 65536 || p->p_grant_q16 > 65536 || p->p_active_q16 > 65536)
    return QE_ERANGE;
  if (p->flags & ~(QE_ELEC_PREVOTE | QE_ELEC_CHECK_QUORUM)) return QE_EINVAL;
  if (p->reserved) return QE_EINVAL;
  if (p->script_resp && (!p->script_grant || p->script_stride < s->num_groups)) return QE_EINVAL;
  EArgs a{};
  a.G = s->num_groups;
  a.goff = s->group_offset;
  a.term = s->term;
  a.state = s->state;
  a.voted = s->voted;
  a.granted = s->granted;
  a.self_slot = s->self_slot;
  a.inc = s->inc_mask;
  a.out = s->out_mask;
  a.learner = s->learner_mask;
  a.seed = p->seed;
  a.step0 = p->step0;
  a.steps = p->steps;
  a.p_drop = p->p_drop_q16;
  a.p_grant = p->p_grant_q16;
  a.flags = p->flags;
  a.p_active = p->p_active_q16;
  a.sresp = p->script_resp;
  a.sgrant = p->script_grant;
  a.shup = p->script_resp ? p->script_hup : nullptr;
  a.sstride = p->script_stride;
  a.stats = stats;
  return with_slots(s->num_slots, [&](auto n) {
    return dispatch_elec<n()>(a, static_cast<hipStream_t>(stream));
  });
}

int qe_apply_append_resps(uint64_t num_groups, uint32_t num_slots, uint64_t stride,
                          uint64_t *match, uint64_t *next, uint64_t n, const uint64_t *group,
                          const int8_t *slot, const uint64_t *index, uint8_t *touched,
                          void *stream) {
  if (num_slots == 0 || num_slots > QE_MAX_SLOTS) return QE_EINVAL;
  if (n == 0 || num_groups == 0) return QE_OK;
  if (stride < num_groups || !match || !next || !group || !slot || !index) return QE_EINVAL;
  hipLaunchKernelGGL(k_apply_acks, dim3(elem_grid(n, num_cus())), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), num_groups, num_slots, stride, match,
                     next, n, group, slot, index, touched);
  return hip_status(hipGetLastError());
}

// The rules every entry point that takes a qe_progress opens with.  (Two
// gaps ADVICE.md lists are not closed here, being behaviour changes:
// qe_switch_config accepts a missing self_slot, and qe_read_index accepts
// read_keys without a key.)
static int check_progress(const qe_progress *p) {
  if (!p) return QE_EINVAL;
  if (p->num_slots == 0 || p->num_slots > QE_MAX_SLOTS || p->reserved || p->reserved2)
    return QE_EINVAL;
  return QE_OK;
}

// the [S][stride] rows hold the batch, and out_mask (a joint configuration)
// comes with inc_mask
static bool bad_rows_or_masks(const qe_progress *p) {
  return (p->num_groups && p->stride < p->num_groups) || (p->out_mask && !p->inc_mask);
}

// ABI 5: the ReadIndex queue comes whole or not at all
static bool partial_read_queue(const qe_progress *p) {
  return p->read_acks && (!p->read_head || !p->read_count);
}

// The ReadIndex queue's ABI 7 fields: a capacity of 0 is QE_READ_QUEUE (the
// ABI 5 queue); a longer queue needs the overflow ring.
static int read_queue_cap(const qe_progress *p, uint32_t *cap) {
  if (p->reserved3) return QE_EINVAL;
  if (p->read_cap != 0 && (p->read_cap < QE_READ_QUEUE || p->read_cap > QE_READ_CAP_MAX))
    return QE_ERANGE;
  *cap = p->read_cap ? p->read_cap : QE_READ_QUEUE;
  if (p->read_acks && *cap > QE_READ_QUEUE && !p->read_ovf) return QE_EINVAL;
  return QE_OK;
}

// The fields of the state more than one kernel reads.  The partial entry
// points validate only part of the struct and still get every field here, so
// their kernels must read only what their entry point checked.  Audited when
// this was introduced: k_heartbeat reads G, stride, match, committed, tracked,
// self_slot and the read_* queue; k_check_quorum reads G, goff, stride, pw,
// inc, out, tracked and self_slot; k_read_index reads G, stride, committed,
// term_start, last_index, inc, out, self_slot and the read_* queue (with
// read_ovf and read_keys).  A kernel edit that reads another field here
// (a.tracked in k_read_index, say) needs the matching check in its entry
// point first.
static void state_args(const qe_progress *p, PArgs &a) {
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.match = p->match;
  a.pw = p->peer;
  a.committed = p->committed;
  a.term_start = p->term_start;
  a.last_index = p->last_index;
  a.inc = p->inc_mask;
  a.out = p->out_mask;
  a.tracked = p->tracked;
  a.self_slot = p->self_slot;
  a.read_acks = p->read_acks;
  a.read_head = p->read_head;
  a.read_count = p->read_count;
  a.read_ovf = p->read_ovf;
  a.read_keys = p->read_keys;
}

static int progress_args(const qe_progress *p, PArgs &a) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (p->inflight_cap == 0 || p->inflight_cap > QE_MAX_INFLIGHT) return QE_ERANGE;
  if (p->log_runs > QE_MAX_LOG_RUNS) return QE_ERANGE;
  if (bad_rows_or_masks(p)) return QE_EINVAL;
  if (p->num_groups &&
      (!p->match || !p->next || !p->pending_snapshot || !p->peer || !p->infl_lo || !p->infl_hi ||
       !p->committed || !p->term_start || !p->first_index || !p->last_index))
    return QE_EINVAL;
  if (p->num_groups && p->log_runs && (!p->run_first || !p->run_term || !p->run_count))
    return QE_EINVAL;
  // a slot's ring block of a 64-group tile is addressed with 32-bit offsets
  if (static_cast<uint64_t>(QE_RING_PITCH(p->inflight_cap)) * 4 * 64 > 0x7FFFFFFFull)
    return QE_ERANGE;
  // ABI 8: the 16-bit Inflights form exists for the pipelined kernels' shapes
  if (p->infl16 && (p->inflight_cap > QE_RING16_MAX_F || p->num_slots > QE_RING16_MAX_SLOTS ||
                    p->log_runs > 4))
    return QE_ERANGE;
  a = PArgs{};
  state_args(p, a);
  a.F = p->inflight_cap;
  a.R = p->log_runs;
  a.next = p->next;
  a.pending = p->pending_snapshot;
  a.ilo = p->infl_lo;
  a.ihi = p->infl_hi;
  a.infl16 = p->infl16;
  a.FP = QE_RING_PITCH(p->inflight_cap);
  a.first_index = p->first_index;
  a.snap_index = p->snap_index;
  a.run_first = p->run_first;
  a.run_term = p->run_term;
  a.run_count = p->run_count;
  a.transferee = p->lead_transferee;
  a.max_ents = p->max_ents;
  return read_queue_cap(p, &a.read_cap);
}

// the launch every Progress entry point ends with
static int launch_progress(const qe_progress *p, const PArgs &a, ProgressOp op, bool acct,
                           void *stream) {
  return with_slots(p->num_slots, [&](auto s) {
    return dispatch_progress<s()>(a, op, acct, p->inc_mask != nullptr, p->out_mask != nullptr,
                                  static_cast<hipStream_t>(stream));
  });
}

int qe_progress_step(const qe_progress *p, const qe_peer_msgs *m, uint64_t *stats,
                     void *stream) {
  PArgs a;
  int rc = progress_args(p, a);
  if (rc) return rc;
  if (!m) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  if (!m->type || !m->index || !m->reject_hint || !m->log_term) return QE_EINVAL;
  if (p->log_runs == 0) return QE_EINVAL;  // findConflictByTerm needs the log model
  a.mtype = m->type;
  a.mindex = m->index;
  a.mhint = m->reject_hint;
  a.mlogterm = m->log_term;
  a.sent = m->sent;
  a.bcast = m->bcast;
  a.snap = m->snap;
  a.tnow = m->timeout_now;
  a.msg_count = m->msg_count;
  a.msg_index = m->msg_index;
  a.acct = m->bytes_requested;
  if (partial_read_queue(p)) return QE_EINVAL;
  a.read_ctx = p->read_acks ? m->read_ctx : nullptr;
  a.read_released = m->read_released;
  a.term_commit = m->term_commit;
  a.term_commit_index = m->term_commit_index;
  a.stats = stats;
  return launch_progress(p, a, ProgressOp::Step, m->bytes_requested != nullptr, stream);
}

int qe_progress_send(const qe_progress *p, const void *want, uint32_t send_if_empty,
                     void *sent, void *snap, void *stream) {
  PArgs a;
  int rc = progress_args(p, a);
  if (rc) return rc;
  if (p->num_groups == 0) return QE_OK;
  if (!want) return QE_EINVAL;
  a.want = want;
  a.send_if_empty = send_if_empty;
  a.sent = sent;
  a.snap = snap;
  return launch_progress(p, a, ProgressOp::Send, false, stream);
}

int qe_propose(const qe_progress *p, const qe_proposals *prop, uint64_t *stats, void *stream) {
  PArgs a;
  int rc = progress_args(p, a);
  if (rc) return rc;
  if (!prop || (prop->flags & ~QE_PROP_APPEND_ONLY)) return QE_EINVAL;
  if (prop->max_cc > QE_PROP_MAX_CC) return QE_ERANGE;
  if (p->num_groups == 0) return QE_OK;
  if (!prop->num_entries || !prop->result) return QE_EINVAL;
  if (!p->self_slot) return QE_EINVAL;  // MsgProp is handled by the leader: its slot is needed
  if (prop->max_cc && (!prop->cc_count || !prop->cc_pos || !prop->cc_leave || !prop->cc_size ||
                       !prop->applied || !prop->pending_conf_index ||
                       prop->cc_stride < p->num_groups))
    return QE_EINVAL;
  if (!prop->uncommitted_size && prop->max_uncommitted) return QE_EINVAL;
  a.prop_n = prop->num_entries;
  a.prop_payload = prop->payload;
  const bool append_only = (prop->flags & QE_PROP_APPEND_ONLY) != 0;
  a.max_cc = append_only ? 0u : prop->max_cc;
  a.prop_flags = prop->flags;
  a.cc_stride = prop->cc_stride;
  a.cc_count = prop->cc_count;
  a.cc_pos = prop->cc_pos;
  a.cc_leave = prop->cc_leave;
  a.cc_size = prop->cc_size;
  a.applied = prop->applied;
  a.pci = prop->pending_conf_index;
  a.unc = prop->uncommitted_size;
  a.max_unc = prop->max_uncommitted;
  a.prop_result = prop->result;
  a.cc_refused = prop->cc_refused;
  a.sent = prop->sent;
  a.snap = prop->snap;
  a.acct = prop->bytes_requested;
  a.last_index_rw = const_cast<uint64_t *>(p->last_index);
  a.stats = stats;
  return launch_progress(p, a, ProgressOp::Propose, prop->bytes_requested != nullptr, stream);
}

int qe_switch_config(const qe_progress *p, const qe_switch *sw, uint64_t *stats, void *stream) {
  PArgs a;
  int rc = progress_args(p, a);
  if (rc) return rc;
  if (!sw) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  if (!sw->result) return QE_EINVAL;
  a.sw_switched = sw->switched;
  a.sw_result = sw->result;
  a.sent = sw->sent;
  a.snap = sw->snap;
  a.acct = sw->bytes_requested;
  a.stats = stats;
  return launch_progress(p, a, ProgressOp::SwitchConfig, sw->bytes_requested != nullptr, stream);
}

int qe_become_leader(const qe_progress *p, const qe_leader *l, uint64_t *stats, void *stream) {
  PArgs a;
  int rc = progress_args(p, a);
  if (rc) return rc;
  if (!l || l->reserved || (l->flags & ~QE_BL_BCAST)) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  if (!l->term || !l->result || !p->self_slot) return QE_EINVAL;
  if (p->log_runs && !p->run_count) return QE_EINVAL;
  a.bl_elected = l->elected;
  a.bl_term = l->term;
  a.bl_flags = l->flags;
  a.bl_pci = l->pending_conf_index;
  a.bl_unc = l->uncommitted_size;
  a.bl_result = l->result;
  a.sent = l->sent;
  a.snap = l->snap;
  a.stats = stats;
  return launch_progress(p, a, ProgressOp::BecomeLeader, false, stream);
}

int qe_heartbeat(const qe_progress *p, uint64_t *commit, uint32_t *ctx, void *sent, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (p->num_groups == 0) return QE_OK;
  if (p->stride < p->num_groups || !p->match || !p->committed || !commit) return QE_EINVAL;
  if (partial_read_queue(p)) return QE_EINVAL;
  PArgs a{};
  state_args(p, a);
  const int rq = read_queue_cap(p, &a.read_cap);
  if (rq) return rq;
  a.hb_commit = commit;
  a.hb_ctx = ctx;
  a.sent = sent;
  return launch_progress(p, a, ProgressOp::Heartbeat, false, stream);
}

int qe_tick(const qe_progress *p, const qe_timers *t, const qe_tick_out *out, uint64_t *stats,
            void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!t || !out) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  if (!t->state || !t->timer || !t->randomized_timeout || !out->action) return QE_EINVAL;
  // 2 * election_timeout - 1 must fit the saturating 16-bit counters
  if (t->election_timeout == 0 || t->election_timeout > 32768u) return QE_EINVAL;
  if (t->heartbeat_timeout == 0 || t->heartbeat_timeout > 65535u) return QE_EINVAL;
  if ((t->flags & ~QE_TICK_CHECK_QUORUM) || t->ticks > 1) return QE_EINVAL;
  if (p->out_mask && !p->inc_mask) return QE_EINVAL;
  const bool checks = (t->flags & QE_TICK_CHECK_QUORUM) && t->ticks == 1;
  if (checks && !p->peer) return QE_EINVAL;
  // the [S][stride] rows it touches: the peer words, Match and hb_commit
  if ((checks || out->hb_commit) && p->stride < p->num_groups) return QE_EINVAL;
  if (out->hb_commit && (!p->match || !p->committed)) return QE_EINVAL;
  if (partial_read_queue(p)) return QE_EINVAL;
  TArgs a{};
  const int rq = read_queue_cap(p, &a.read_cap);  // (the capacity rules are qe_heartbeat's)
  if (rq) return rq;
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.state = t->state;
  a.timer = t->timer;
  a.rt = t->randomized_timeout;
  a.no_campaign = t->no_campaign;
  a.events = t->events;
  a.et = t->election_timeout;
  a.ht = t->heartbeat_timeout;
  a.flags = t->flags;
  a.ticks = t->ticks;
  a.seed = t->seed;
  a.tick_no = static_cast<uint32_t>(t->tick_no);
  a.pw = p->peer;
  a.match = p->match;
  a.committed = p->committed;
  a.inc = p->inc_mask;
  a.out = p->out_mask;
  a.tracked = p->tracked;
  a.self_slot = p->self_slot;
  a.transferee = p->lead_transferee;
  a.read_acks = p->read_acks;
  a.read_head = p->read_head;
  a.read_count = p->read_count;
  a.action = out->action;
  a.hb_commit = out->hb_commit;
  a.hb_ctx = out->hb_ctx;
  a.hb_sent = out->hb_sent;
  a.qactive = out->quorum_active;
  a.stats = stats;
  return with_slots(p->num_slots, [&](auto s) {
    return dispatch_tick<s()>(a, p->inc_mask != nullptr, p->out_mask != nullptr,
                              static_cast<hipStream_t>(stream));
  });
}

// What the step entry points (qe_follower_step, qe_vote_step, qe_snapshot_step,
// qe_compact) ask of their arguments alike.  The term-run log model: the run
// table with its count and last_index, and committed for all but the vote,
// in rows that hold the batch.
static bool missing_log_model(const qe_progress *p, bool committed = true) {
  return p->log_runs == 0 || p->log_runs > QE_MAX_LOG_RUNS || (committed && !p->committed) ||
         !p->last_index || !p->run_first || !p->run_term || !p->run_count ||
         p->stride < p->num_groups;
}
// The qe_follower header rows; `vote` is optional except to qe_vote_step.
static bool missing_follower(const qe_follower *f, bool vote = false) {
  return !f->term || !f->state || !f->lead || (vote && !f->vote);
}

int qe_follower_step(const qe_progress *p, const qe_follower *f, const qe_leader_msgs *m,
                     const qe_follower_out *out, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !m || !out) return QE_EINVAL;
  if ((f->flags & ~(QE_FOLLOW_CHECK_QUORUM | QE_FOLLOW_PREVOTE)) || f->reserved || m->reserved)
    return QE_EINVAL;
  if (m->msg_runs > QE_MAX_MSG_RUNS || missing_log_model(p)) return QE_EINVAL;
  if (missing_follower(f) || !out->result) return QE_EINVAL;
  if (!m->type || !m->from || !m->term || !m->index || !m->log_term || !m->commit)
    return QE_EINVAL;
  if (m->msg_runs && (!m->ent_len || !m->ent_term)) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  FArgs a{};
  step_head(p, stats, a);
  a.E = m->msg_runs;
  a.S = p->num_slots;
  a.flags = f->flags;
  // the log rows are const in qe_progress for the leader's entry points; the
  // follower appends to them (as qe_propose / qe_become_leader do)
  a.committed = p->committed;
  a.last_index = const_cast<uint64_t *>(p->last_index);
  a.run_first = const_cast<uint64_t *>(p->run_first);
  a.run_term = const_cast<uint64_t *>(p->run_term);
  a.run_count = const_cast<uint8_t *>(p->run_count);
  a.transferee = p->lead_transferee;
  a.term = f->term;
  a.state = f->state;
  a.lead = f->lead;
  a.vote = f->vote;
  a.type = m->type;
  a.from = m->from;
  a.mterm = m->term;
  a.index = m->index;
  a.log_term = m->log_term;
  a.commit = m->commit;
  a.ent_len = m->ent_len;
  a.ent_term = m->ent_term;
  a.result = out->result;
  a.resp_index = out->resp_index;
  a.reject_hint = out->reject_hint;
  a.resp_log_term = out->resp_log_term;
  a.append_from = out->append_from;
  a.events = out->events;
  return dispatch_follow(a, static_cast<hipStream_t>(stream));
}

int qe_vote_step(const qe_progress *p, const qe_follower *f, const qe_voter *v,
                 const qe_vote_msgs *m, const qe_vote_out *out, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !v || !m || !out) return QE_EINVAL;
  if (v->flags & ~(QE_VOTE_CHECK_QUORUM | QE_VOTE_PREVOTE)) return QE_EINVAL;
  if ((v->flags & QE_VOTE_CHECK_QUORUM) && !v->timer) return QE_EINVAL;
  // the saturating 16-bit electionElapsed compares exactly up to here
  if (v->election_timeout == 0 || v->election_timeout > 32768u) return QE_EINVAL;
  if (!v->voted != !v->granted) return QE_EINVAL;
  if (p->out_mask && !p->inc_mask) return QE_EINVAL;
  if (missing_log_model(p, false)) return QE_EINVAL;
  if (missing_follower(f, true) || !out->result) return QE_EINVAL;
  if (!m->type || !m->from || !m->term || !m->index || !m->log_term) return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  VArgs a{};
  step_head(p, stats, a);
  a.S = p->num_slots;
  a.et = v->election_timeout;
  a.flags = v->flags;
  a.last_index = p->last_index;
  a.run_term = p->run_term;
  a.run_count = p->run_count;
  a.inc = p->inc_mask;
  a.out = p->out_mask;
  a.tracked = p->tracked;
  a.self_slot = p->self_slot;
  a.transferee = p->lead_transferee;
  a.term = f->term;
  a.state = f->state;
  a.lead = f->lead;
  a.vote = f->vote;
  a.timer = v->timer;
  a.voted = v->voted;
  a.granted = v->granted;
  a.no_campaign = v->no_campaign;
  a.type = m->type;
  a.from = m->from;
  a.mterm = m->term;
  a.index = m->index;
  a.log_term = m->log_term;
  a.mflags = m->flags;
  a.result = out->result;
  a.resp_term = out->resp_term;
  a.req_log_term = out->req_log_term;
  a.req_to = out->req_to;
  a.elected = out->elected;
  a.events = out->events;
  return dispatch_vote(a, static_cast<hipStream_t>(stream));
}

int qe_compact(const qe_progress *p, const qe_compaction *c, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!c || !c->compact_index || !c->result) return QE_EINVAL;
  if (missing_log_model(p)) return QE_EINVAL;
  if (c->create_index && !p->snap_index) return QE_EINVAL;  // CreateSnapshot records it there
  if (p->num_groups == 0) return QE_OK;
  CPArgs a{};
  step_head(p, stats, a);
  a.committed = p->committed;
  a.last_index = p->last_index;
  // const in qe_progress for the leader's entry points (as in qe_follower_step)
  a.run_first = const_cast<uint64_t *>(p->run_first);
  a.run_term = const_cast<uint64_t *>(p->run_term);
  a.run_count = const_cast<uint8_t *>(p->run_count);
  a.first_index = const_cast<uint64_t *>(p->first_index);
  a.snap_index = const_cast<uint64_t *>(p->snap_index);
  a.compact_index = c->compact_index;
  a.create_index = c->create_index;
  a.applied = c->applied;
  a.snap_term = c->snap_term;
  a.result = c->result;
  return dispatch_compact(a, static_cast<hipStream_t>(stream));
}

// the configuration a restore rewrites is the batch's own
static bool conf_mismatch(const qe_progress *p, const qe_conf *c) {
  return c->num_groups != p->num_groups || c->num_slots != p->num_slots || c->reserved != 0;
}

int qe_snapshot_step(const qe_progress *p, const qe_follower *f, const qe_conf *c,
                     const qe_snap_msgs *m, const qe_snap_out *out, uint64_t *stats,
                     void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !c || !m || !out) return QE_EINVAL;
  if (conf_mismatch(p, c)) return QE_EINVAL;
  if (missing_log_model(p)) return QE_EINVAL;
  if (!p->self_slot) return QE_EINVAL;  // restore() looks for the receiver in the ConfState
  if (missing_follower(f) || !out->result) return QE_EINVAL;
  if (!m->type || !m->from || !m->term || !m->snap_index || !m->snap_term || !m->cs_inc ||
      !m->cs_out || !m->cs_learner || !m->cs_learners_next || !m->cs_auto_leave)
    return QE_EINVAL;
  if (p->num_groups == 0) return QE_OK;
  SNArgs a{};
  step_head(p, stats, a);
  a.S = p->num_slots;
  a.committed = p->committed;
  a.last_index = const_cast<uint64_t *>(p->last_index);
  a.run_first = const_cast<uint64_t *>(p->run_first);
  a.run_term = const_cast<uint64_t *>(p->run_term);
  a.run_count = const_cast<uint8_t *>(p->run_count);
  a.first_index = const_cast<uint64_t *>(p->first_index);
  a.snap_index = const_cast<uint64_t *>(p->snap_index);
  a.self_slot = p->self_slot;
  a.transferee = p->lead_transferee;
  a.term = f->term;
  a.state = f->state;
  a.lead = f->lead;
  a.vote = f->vote;
  a.slot_ids = c->slot_ids;
  a.c_inc = c->inc_mask;
  a.c_out = c->out_mask;
  a.c_lrn = c->learner_mask;
  a.c_lnx = c->learners_next_mask;
  a.c_isl = c->is_learner;
  a.c_trk = c->tracked;
  a.c_auto = c->auto_leave;
  a.type = m->type;
  a.from = m->from;
  a.mterm = m->term;
  a.sindex = m->snap_index;
  a.sterm = m->snap_term;
  a.m_inc = m->cs_inc;
  a.m_out = m->cs_out;
  a.m_lrn = m->cs_learner;
  a.m_lnx = m->cs_learners_next;
  a.m_auto = m->cs_auto_leave;
  a.m_ids = m->cs_ids;
  a.result = out->result;
  a.resp_index = out->resp_index;
  a.events = out->events;
  return dispatch_snap(a, static_cast<hipStream_t>(stream));
}

int qe_read_index(const qe_progress *p, const uint8_t *request, const uint64_t *key,
                  uint32_t lease_based, uint8_t *result, uint32_t *ctx, uint64_t *index,
                  void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (p->num_groups == 0) return QE_OK;
  if (bad_rows_or_masks(p) || !request || !result) return QE_EINVAL;
  if (!p->committed || !p->term_start || !p->last_index) return QE_EINVAL;
  // ReadOnlySafe queues: the queue must be there
  if (!lease_based && (!p->read_acks || !p->read_head || !p->read_count)) return QE_EINVAL;
  PArgs a{};
  state_args(p, a);
  const int rq = read_queue_cap(p, &a.read_cap);
  if (rq) return rq;
  a.ri_key = p->read_keys ? key : nullptr;  // keys are checked only when the state keeps them
  a.ri_request = request;
  a.ri_result = result;
  a.ri_ctx = ctx;
  a.ri_index = index;
  a.lease_based = lease_based ? 1u : 0u;
  return launch_progress(p, a, ProgressOp::ReadIndex, false, stream);
}

int qe_check_quorum(const qe_progress *p, uint8_t *quorum_active, uint64_t *stats,
                    void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (p->num_groups == 0) return QE_OK;
  if (bad_rows_or_masks(p) || !p->peer) return QE_EINVAL;
  PArgs a{};
  state_args(p, a);
  a.qactive = quorum_active;
  a.stats = stats;
  return launch_progress(p, a, ProgressOp::CheckQuorum, false, stream);
}

int qe_confchange(const qe_conf *c, const qe_conf_changes *ch, const qe_progress *p,
                  void *stream) {
  if (!c || !ch) return QE_EINVAL;
  if (c->num_slots == 0 || c->num_slots > QE_MAX_SLOTS || c->reserved) return QE_EINVAL;
  if (c->num_groups == 0) return QE_OK;
  if (!c->slot_ids || !c->inc_mask || !c->out_mask || !c->learner_mask ||
      !c->learners_next_mask || !c->is_learner || !c->tracked || !c->auto_leave)
    return QE_EINVAL;
  if (!ch->op || !ch->count || !ch->last_index || !ch->result) return QE_EINVAL;
  if (ch->max_changes > 255) return QE_EINVAL;  // count is a u8 per group
  if (ch->max_changes > 0 && (!ch->type || !ch->node_id || ch->stride < c->num_groups))
    return QE_EINVAL;
  CCArgs a{};
  a.G = c->num_groups;
  a.C = ch->max_changes;
  a.stride = ch->stride;
  a.ids = c->slot_ids;
  a.inc = c->inc_mask;
  a.out = c->out_mask;
  a.lrn = c->learner_mask;
  a.lnx = c->learners_next_mask;
  a.isl = c->is_learner;
  a.trk = c->tracked;
  a.auto_leave = c->auto_leave;
  a.op = ch->op;
  a.count = ch->count;
  a.type = ch->type;
  a.node = ch->node_id;
  a.last_index = ch->last_index;
  a.result = ch->result;
  a.new_progress = ch->new_progress;
  if (p) {
    if (p->num_groups != c->num_groups || p->num_slots != c->num_slots ||
        p->stride < p->num_groups)
      return QE_EINVAL;
    if (!p->match || !p->next || !p->pending_snapshot || !p->peer) return QE_EINVAL;
    a.pstride = p->stride;
    a.p_match = p->match;
    a.p_next = p->next;
    a.p_pending = p->pending_snapshot;
    a.p_pw = p->peer;
  }
  // chunks of up to kCCTPW tiles per wave (the chunk plan of qe_launch.hpp;
  // a tiles_per_wave override is floored at 2 too)
  const ChunkPlan plan =
      chunk_plan((a.G + 63) / 64, num_cus(), g_tiles_per_wave, kCCTPW, true);
  if (plan.status) return plan.status;
  a.chunk = plan.chunk;
  return with_slots(c->num_slots, [&](auto s) {
    hipLaunchKernelGGL(k_confchange<s()>, dim3(plan.blocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a);
    return hip_status(hipGetLastError());
  });
}

// qe_apply_conf's scratch: the `switched` row, then the switch kernel's result
// row for a call without sw, each padded to 16 B.
static size_t apply_conf_row_bytes(uint64_t num_groups) {
  return (static_cast<size_t>(num_groups) + 15) & ~static_cast<size_t>(15);
}

size_t qe_apply_conf_scratch_bytes(uint64_t num_groups) {
  return 2 * apply_conf_row_bytes(num_groups);
}

int qe_apply_conf(const qe_progress *p, const qe_follower *f, const qe_conf *c,
                  const qe_apply_conf_in *in, const qe_apply_conf_out *out, const qe_switch *sw,
                  void *scratch, void *stream) {
  PArgs pa;
  const int rc = progress_args(p, pa);  // the switch kernel's own checks
  if (rc) return rc;
  if (!f || !c || !in || !out) return QE_EINVAL;
  if (!f->state || !p->inc_mask || !p->out_mask || !p->tracked || !p->self_slot) return QE_EINVAL;
  if (conf_mismatch(p, c)) return QE_EINVAL;
  if (!c->slot_ids || !c->inc_mask || !c->out_mask || !c->learner_mask ||
      !c->learners_next_mask || !c->is_learner || !c->tracked || !c->auto_leave)
    return QE_EINVAL;
  if (in->reserved || in->max_changes > 255) return QE_EINVAL;
  if (in->capacity && (!in->group || !in->transition || !in->num_changes ||
                       (in->max_changes && (!in->type || !in->node_id))))
    return QE_EINVAL;
  if (in->capacity && (!out->result || !out->cc_result || !out->sw_result || !out->inc ||
                       !out->out || !out->learner || !out->learners_next || !out->tracked ||
                       !out->new_progress || !out->auto_leave))
    return QE_EINVAL;
  if (sw && (!sw->result || sw->bytes_requested)) return QE_EINVAL;
  if (!scratch || !al(scratch, 16)) return QE_EINVAL;
  if (p->num_groups == 0 || in->capacity == 0) return QE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t row = apply_conf_row_bytes(p->num_groups);
  uint8_t *switched = static_cast<uint8_t *>(scratch);
  uint8_t *swres = sw ? sw->result : switched + row;
  ACArgs a{};
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.pstride = p->stride;
  a.cap = in->capacity;
  a.n = in->n < in->capacity ? in->n : in->capacity;
  a.count = in->count;
  a.C = in->max_changes;
  a.ids = c->slot_ids;
  a.inc = c->inc_mask;
  a.out = c->out_mask;
  a.lrn = c->learner_mask;
  a.lnx = c->learners_next_mask;
  a.isl = c->is_learner;
  a.trk = c->tracked;
  a.auto_leave = c->auto_leave;
  // p's rows of the configuration, where they are not c's own
  a.p_inc = p->inc_mask != c->inc_mask ? const_cast<void *>(p->inc_mask) : nullptr;
  a.p_out = p->out_mask != c->out_mask ? const_cast<void *>(p->out_mask) : nullptr;
  a.p_trk = p->tracked != c->tracked ? const_cast<void *>(p->tracked) : nullptr;
  a.p_match = p->match;
  a.p_next = p->next;
  a.p_pending = p->pending_snapshot;
  a.p_pw = p->peer;
  a.last_index = p->last_index;
  a.fstate = f->state;
  a.group = in->group;
  a.transition = in->transition;
  a.nchanges = in->num_changes;
  a.type = in->type;
  a.node = in->node_id;
  a.slot = in->slot;
  a.result = out->result;
  a.cc_result = out->cc_result;
  a.sw_result = out->sw_result;
  a.o_inc = out->inc;
  a.o_out = out->out;
  a.o_lrn = out->learner;
  a.o_lnx = out->learners_next;
  a.o_trk = out->tracked;
  a.o_newp = out->new_progress;
  a.o_al = out->auto_leave;
  a.o_ids = out->ids;
  a.switched = switched;
  a.swres = swres;
  int s = dispatch_apply_conf_clear(switched, row, st);
  if (s) return s;
  s = dispatch_apply_conf(a, p->num_slots, st);
  if (s) return s;
  // switchToConfig's leader half, by qe_switch_config's kernel and dispatch
  pa.sw_switched = switched;
  pa.sw_result = swres;
  pa.sent = sw ? sw->sent : nullptr;
  pa.snap = sw ? sw->snap : nullptr;
  s = launch_progress(p, pa, ProgressOp::SwitchConfig, false, stream);
  if (s) return s;
  return dispatch_apply_conf_gather(a, st);
}

size_t qe_collect_scratch_bytes(uint64_t num_groups) {
  return static_cast<size_t>(scan_chunks(num_groups) * (sizeof(uint32_t) + sizeof(uint64_t)) + 64);
}

int qe_collect(uint64_t num_groups, uint64_t group_offset, const uint64_t *perm,
               const uint8_t *flags, const uint64_t *values, uint64_t *out_groups,
               uint64_t *out_values, uint64_t *out_count, void *scratch, void *stream) {
  if (!out_count || (num_groups && (!flags || !scratch))) return QE_EINVAL;
  if (out_values && !values) return QE_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (num_groups == 0)
    return hip_status(hipMemsetAsync(out_count, 0, sizeof(uint64_t), st));
  const ScanScratch sc = scan_scratch(scratch, num_groups);
  if (sc.status) return sc.status;
  if (!al(scratch, 8)) return QE_EINVAL;
  launch_count(flags, num_groups, sc, st);
  if (const int s = launch_scan(sc, out_count, st)) return s;
  hipLaunchKernelGGL(k_collect_scatter, dim3(static_cast<unsigned>(sc.nb)), dim3(kBlock), 0, st,
                     flags, num_groups, al(flags, 16), group_offset, perm, values, sc.offsets,
                     out_groups, out_values);
  return hip_status(hipGetLastError());
}

size_t qe_outbox_scratch_bytes(uint64_t num_groups) {
  return qe_collect_scratch_bytes(num_groups);
}

int qe_outbox(const qe_progress *p, const qe_outbox_in *in, const qe_outbox_out *out,
              void *scratch,
              uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!in || !out || !out->count || !in->term) return QE_EINVAL;
  if (in->reserved || out->reserved || p->reserved3) return QE_EINVAL;
  if (missing_log_model(p)) return QE_EINVAL;
  if (in->sent && !in->index && !in->next_before) return QE_EINVAL;
  if (in->sent && !in->index && (!p->next || !p->peer)) return QE_EINVAL;  // next_before is used
  if (in->snap && !p->snap_index && !p->first_index) return QE_EINVAL;
  if (in->hb_sent && !in->hb_commit) return QE_EINVAL;
  if (out->msg_runs > QE_MAX_MSG_RUNS || (out->msg_runs && (!out->ent_len || !out->ent_term)))
    return QE_EINVAL;
  if (out->capacity && (!out->group || !out->to || !out->type || !out->term || !out->index ||
                        !out->log_term || !out->commit))
    return QE_EINVAL;
  if (p->num_groups && (!scratch || !al(scratch, 8))) return QE_EINVAL;
  const ScanScratch sc = scan_scratch(scratch, p->num_groups);
  if (sc.status) return sc.status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0) return hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
  OBArgs a{};
  step_head(p, stats, a);
  a.S = p->num_slots;
  a.wide = p->num_slots > 8;
  a.max_entries = in->max_entries;
  a.nb = sc.nb;
  a.offsets = sc.offsets;
  a.counts = sc.counts;
  a.sent = in->sent;
  a.snap = in->snap;
  a.hb_sent = in->hb_sent;
  a.committed = p->committed;
  a.last_index = p->last_index;
  a.run_first = p->run_first;
  a.run_term = p->run_term;
  a.run_count = p->run_count;
  a.next = p->next;
  a.peer = p->peer;
  a.snap_src = p->snap_index ? p->snap_index : p->first_index;
  a.snap_sub = p->snap_index ? 0 : 1;
  a.index = in->index;
  a.next_before = in->next_before;
  a.term = in->term;
  a.snap_term = in->snap_term;
  a.hb_commit = in->hb_commit;
  a.hb_ctx = in->hb_ctx;
  a.cap = out->capacity;
  a.o_group = out->group;
  a.o_to = out->to;
  a.o_type = out->type;
  a.o_term = out->term;
  a.o_index = out->index;
  a.o_log_term = out->log_term;
  a.o_commit = out->commit;
  a.o_ctx = out->ctx;
  a.o_ent_len = out->ent_len;
  a.o_ent_term = out->ent_term;
  int s = dispatch_outbox_count(a, st);
  if (s) return s;
  s = launch_scan(sc, out->count, st);
  if (s) return s;
  return dispatch_outbox_fill(a, out->msg_runs, st);
}

size_t qe_replies_scratch_bytes(uint64_t num_groups) {
  return qe_collect_scratch_bytes(num_groups);
}

int qe_replies(const qe_progress *p, const qe_replies_in *in, const qe_replies_out *out,
               void *scratch, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!in || !out || !out->count || !in->term) return QE_EINVAL;
  if (in->reserved[0] || in->reserved[1] || p->reserved3) return QE_EINVAL;
  if (p->stride < p->num_groups) return QE_EINVAL;
  if (in->f_result &&
      (!in->f_from || !in->f_resp_index || !in->f_reject_hint || !in->f_resp_log_term))
    return QE_EINVAL;
  if (in->s_result && (!in->s_from || !in->s_resp_index)) return QE_EINVAL;
  if (in->v_result && (!in->v_type || !in->v_from || !in->v_resp_term || !in->v_req_log_term ||
                       !in->v_req_to || !p->last_index))
    return QE_EINVAL;
  if (out->capacity && (!out->group || !out->to || !out->type || !out->term || !out->index ||
                        !out->log_term || !out->hint))
    return QE_EINVAL;
  if (!al(scratch, 8) || (p->num_groups && !scratch)) return QE_EINVAL;
  const ScanScratch sc = scan_scratch(scratch, p->num_groups);
  if (sc.status) return sc.status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0 ||
      (!in->f_result && !in->s_result && !in->v_result && !in->timeout_now))
    return hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
  RPArgs a{};
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.S = p->num_slots;
  a.wide = p->num_slots > 8;
  a.nb = sc.nb;
  a.offsets = sc.offsets;
  a.counts = sc.counts;
  a.term = in->term;
  a.f_result = in->f_result;
  a.f_from = in->f_from;
  a.f_resp_index = in->f_resp_index;
  a.f_reject_hint = in->f_reject_hint;
  a.f_resp_log_term = in->f_resp_log_term;
  a.f_ctx = in->f_ctx;
  a.s_result = in->s_result;
  a.s_from = in->s_from;
  a.s_resp_index = in->s_resp_index;
  a.v_result = in->v_result;
  a.v_type = in->v_type;
  a.v_from = in->v_from;
  a.v_resp_term = in->v_resp_term;
  a.v_req_log_term = in->v_req_log_term;
  a.v_req_to = in->v_req_to;
  a.last_index = p->last_index;
  a.timeout_now = in->timeout_now;
  a.cap = out->capacity;
  a.o_group = out->group;
  a.o_to = out->to;
  a.o_type = out->type;
  a.o_term = out->term;
  a.o_index = out->index;
  a.o_log_term = out->log_term;
  a.o_hint = out->hint;
  a.o_ctx = out->ctx;
  a.o_flags = out->flags;
  a.stats = stats;
  int s = dispatch_replies_count(a, st);
  if (s) return s;
  s = launch_scan(sc, out->count, st);
  if (s) return s;
  return dispatch_replies_fill(a, st);
}

static bool missing_ready_state(const qe_ready_state *rs) {
  return !rs->stable || !rs->applied || !rs->snap_pending || !rs->prev_term || !rs->prev_commit ||
         !rs->prev_vote || !rs->prev_lead || !rs->prev_state;
}
// the field arrays of a record list (the run arrays go with ent_runs)
static bool missing_ready_fields(const qe_ready_out *o) {
  return !o->group || !o->term || !o->commit || !o->vote || !o->lead || !o->state || !o->flags ||
         !o->ent_first || !o->ent_count || !o->ent_last_term || !o->apply_first ||
         !o->apply_count || !o->snap_index;
}

int qe_ready_note(const qe_progress *p, const qe_ready_state *rs, const qe_ready_note_in *in,
                  void *stream) {
  if (!p || !rs || !in || !rs->stable) return QE_EINVAL;
  if (!in->follow_result != !in->append_from) return QE_EINVAL;
  if (!in->snap_result != !in->snap_resp_index) return QE_EINVAL;
  if (in->snap_result && !rs->snap_pending) return QE_EINVAL;
  if (p->num_groups == 0 || (!in->follow_result && !in->snap_result)) return QE_OK;
  RNArgs a{};
  a.G = p->num_groups;
  a.follow_result = in->follow_result;
  a.append_from = in->append_from;
  a.snap_result = in->snap_result;
  a.resp_index = in->snap_resp_index;
  a.stable = rs->stable;
  a.snap_pending = rs->snap_pending;
  return dispatch_ready_note(a, static_cast<hipStream_t>(stream));
}

// qe_collect's part (offsets u64, counts u32), then one flag byte per group
// from a 16-B boundary on.
static size_t ready_flag_offset(uint64_t num_groups) {
  return (qe_collect_scratch_bytes(num_groups) + 15) & ~static_cast<size_t>(15);
}

size_t qe_ready_scratch_bytes(uint64_t num_groups) {
  return ready_flag_offset(num_groups) + static_cast<size_t>(num_groups) + 16;
}

int qe_ready(const qe_progress *p, const qe_follower *f, const qe_ready_state *rs,
             const qe_ready_in *in, const qe_ready_out *out, void *scratch, uint64_t *stats,
             void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !rs || !in || !out || !out->count) return QE_EINVAL;
  if (in->reserved || out->reserved || p->reserved3) return QE_EINVAL;
  if (missing_log_model(p) || missing_follower(f) || missing_ready_state(rs)) return QE_EINVAL;
  if (out->ent_runs > QE_MAX_MSG_RUNS ||
      (out->ent_runs && (!out->ent_len || !out->ent_term || !out->apply_len || !out->apply_term)))
    return QE_EINVAL;
  if (out->capacity && missing_ready_fields(out)) return QE_EINVAL;
  if (!al(scratch, 8) || (p->num_groups && !scratch)) return QE_EINVAL;
  const ScanScratch sc = scan_scratch(scratch, p->num_groups);
  if (sc.status) return sc.status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0) return hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
  RDArgs a{};
  step_head(p, stats, a);
  a.S = p->num_slots;
  a.max_apply = in->max_apply;
  a.nb = sc.nb;
  a.offsets = sc.offsets;
  a.counts = sc.counts;
  a.committed = p->committed;
  a.last_index = p->last_index;
  a.run_first = p->run_first;
  a.run_term = p->run_term;
  a.run_count = p->run_count;
  a.term = f->term;
  a.state = f->state;
  a.lead = f->lead;
  a.vote = f->vote;
  a.stable = rs->stable;
  a.applied = rs->applied;
  a.snap_pending = rs->snap_pending;
  a.prev_term = rs->prev_term;
  a.prev_commit = rs->prev_commit;
  a.prev_vote = rs->prev_vote;
  a.prev_lead = rs->prev_lead;
  a.prev_state = rs->prev_state;
  a.pending = in->pending;
  a.cap = out->capacity;
  a.o_group = out->group;
  a.o_term = out->term;
  a.o_commit = out->commit;
  a.o_vote = out->vote;
  a.o_lead = out->lead;
  a.o_state = out->state;
  a.o_flags = out->flags;
  a.o_ent_first = out->ent_first;
  a.o_ent_count = out->ent_count;
  a.o_ent_last_term = out->ent_last_term;
  a.o_apply_first = out->apply_first;
  a.o_apply_count = out->apply_count;
  a.o_snap_index = out->snap_index;
  a.o_ent_len = out->ent_len;
  a.o_ent_term = out->ent_term;
  a.o_apply_len = out->apply_len;
  a.o_apply_term = out->apply_term;
  // the pair loads of the count pass: 16 B of every u64 row, 2 B of every byte row
  a.vec = al(a.term, 16) && al(a.committed, 16) && al(a.last_index, 16) && al(a.run_first, 16) &&
          al(a.stable, 16) && al(a.applied, 16) && al(a.snap_pending, 16) &&
          al(a.prev_term, 16) && al(a.prev_commit, 16) && al(a.vote, 2) && al(a.lead, 2) &&
          al(a.state, 2) && al(a.prev_vote, 2) && al(a.prev_lead, 2) && al(a.prev_state, 2) &&
          al(a.pending, 2);
  // the flags, behind the offsets and the counts
  const uintptr_t fl = reinterpret_cast<uintptr_t>(scratch) + ready_flag_offset(p->num_groups);
  a.flag = reinterpret_cast<uint8_t *>((fl + 15) & ~static_cast<uintptr_t>(15));
  int s = dispatch_ready_count(a, st);
  if (s) return s;
  s = launch_scan(sc, out->count, st);
  if (s) return s;
  return dispatch_ready_fill(a, out->ent_runs, st);
}

int qe_advance(const qe_progress *p, const qe_follower *f, const qe_ready_state *rs,
               const qe_ready_out *list, const qe_advance_opt *opt, uint8_t *result,
               void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!rs || !list || !list->count || !result) return QE_EINVAL;
  if (list->reserved || p->reserved3 || (opt && (opt->reserved[0] || opt->reserved[1])))
    return QE_EINVAL;
  if (missing_log_model(p) || missing_ready_state(rs)) return QE_EINVAL;
  if (list->capacity && missing_ready_fields(list)) return QE_EINVAL;
  const bool al_on = opt && opt->auto_leave;
  if (al_on && (!opt->pending_conf_index || !f || !f->state)) return QE_EINVAL;
  if (p->num_groups == 0 || list->capacity == 0) return QE_OK;
  ADArgs a{};
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.cap = list->capacity;
  a.R = p->log_runs;
  a.S = p->num_slots;
  a.count = list->count;
  a.group = list->group;
  a.term = list->term;
  a.commit = list->commit;
  a.vote = list->vote;
  a.lead = list->lead;
  a.state = list->state;
  a.flags = list->flags;
  a.ent_first = list->ent_first;
  a.ent_count = list->ent_count;
  a.ent_last_term = list->ent_last_term;
  a.apply_first = list->apply_first;
  a.apply_count = list->apply_count;
  a.snap_index = list->snap_index;
  a.committed = p->committed;
  a.last_index = p->last_index;
  a.run_first = p->run_first;
  a.run_term = p->run_term;
  a.run_count = p->run_count;
  a.stable = rs->stable;
  a.applied = rs->applied;
  a.snap_pending = rs->snap_pending;
  a.prev_term = rs->prev_term;
  a.prev_commit = rs->prev_commit;
  a.prev_vote = rs->prev_vote;
  a.prev_lead = rs->prev_lead;
  a.prev_state = rs->prev_state;
  a.auto_leave = al_on ? opt->auto_leave : nullptr;
  a.pending_conf_index = al_on ? opt->pending_conf_index : nullptr;
  a.cur_state = al_on ? f->state : nullptr;
  a.result = result;
  return dispatch_advance(a, static_cast<hipStream_t>(stream));
}

int qe_read_note(const qe_progress *p, const qe_read_book *b, const uint8_t *result,
                 const uint32_t *ctx, const uint64_t *index, const uint8_t *from, void *stream) {
  if (!p || !b || !result || !ctx || !index || !b->req_index || !b->req_from) return QE_EINVAL;
  RNoteArgs a{};
  const int rq = read_queue_cap(p, &a.cap);
  if (rq) return rq;
  if (p->num_groups == 0) return QE_OK;
  a.G = p->num_groups;
  a.result = result;
  a.ctx = ctx;
  a.index = index;
  a.from = from;
  a.req_index = b->req_index;
  a.req_from = b->req_from;
  return dispatch_read_note(a, static_cast<hipStream_t>(stream));
}

size_t qe_read_states_scratch_bytes(uint64_t num_groups) {
  return qe_collect_scratch_bytes(num_groups);
}

int qe_read_states(const qe_progress *p, const qe_read_book *b, const qe_read_states_in *in,
                   const qe_read_states_out *out, void *scratch, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!in || !out || !out->count) return QE_EINVAL;
  if (in->reserved[0] || in->reserved[1]) return QE_EINVAL;
  // the released requests are looked up in the book, from the queue's head on
  if (in->read_released &&
      (!b || !b->req_index || !b->req_from || !p->read_head || !p->read_count))
    return QE_EINVAL;
  if ((in->term_commit && !in->term_commit_index) || (in->ri_result && !in->ri_index))
    return QE_EINVAL;
  if (out->capacity && (!out->group || !out->kind || !out->to || !out->ctx || !out->index))
    return QE_EINVAL;
  if (!al(scratch, 8) || (p->num_groups && !scratch)) return QE_EINVAL;
  RSArgs a{};
  const int rq = read_queue_cap(p, &a.cap);
  if (rq) return rq;
  const ScanScratch sc = scan_scratch(scratch, p->num_groups);
  if (sc.status) return sc.status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0 || (!in->read_released && !in->term_commit && !in->ri_result))
    return hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.S = p->num_slots;
  a.nb = sc.nb;
  a.offsets = sc.offsets;
  a.counts = sc.counts;
  a.read_released = in->read_released;
  a.term_commit = in->term_commit;
  a.term_commit_index = in->term_commit_index;
  a.ri_result = in->ri_result;
  a.ri_index = in->ri_index;
  a.ri_from = in->ri_from;
  a.ri_key = in->ri_key;
  a.read_head = p->read_head;
  a.self_slot = p->self_slot;
  a.read_keys = p->read_keys;
  a.req_index = b ? b->req_index : nullptr;
  a.req_from = b ? b->req_from : nullptr;
  a.ocap = out->capacity;
  a.o_group = out->group;
  a.o_kind = out->kind;
  a.o_to = out->to;
  a.o_ctx = out->ctx;
  a.o_index = out->index;
  a.o_key = out->key;
  a.stats = stats;
  int s = dispatch_read_states_count(a, st);
  if (s) return s;
  s = launch_scan(sc, out->count, st);
  if (s) return s;
  return dispatch_read_states_fill(a, st);
}

size_t qe_inbox_scratch_bytes(uint64_t num_groups, uint32_t num_slots, uint64_t num_records) {
  if (num_slots == 0 || num_slots > QE_MAX_SLOTS) return 0;
  IBArgs a{num_groups, 0, 0, num_records, num_slots};  // (G, goff, stride, n, S)
  ScanScratch sc;
  return inbox_scratch(nullptr, a, sc);
}

int qe_inbox(const qe_progress *p, const qe_follower *f, const qe_inbox_in *in,
             const qe_inbox_out *out, void *scratch, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !in || !out || !f->term || !f->state) return QE_EINVAL;
  if (in->reserved) return QE_EINVAL;
  if (p->num_groups && p->stride < p->num_groups) return QE_EINVAL;
  if (in->msg_runs > QE_MAX_MSG_RUNS ||
      (in->msg_runs && (!in->ent_len || !in->ent_term || !out->f_ent_len || !out->f_ent_term)))
    return QE_EINVAL;
  const uint64_t n = in->num_records;
  if (n && (!in->group || !in->from || !in->type || !in->term || !in->index || !in->log_term ||
            !in->commit || !in->hint))
    return QE_EINVAL;
  if (!out->f_type || !out->f_from || !out->f_term || !out->f_index || !out->f_log_term ||
      !out->f_commit || !out->s_type || !out->s_from || !out->s_term || !out->s_snap_index ||
      !out->s_snap_term || !out->v_type || !out->v_from || !out->v_term || !out->v_index ||
      !out->v_log_term || !out->r_type || !out->r_index || !out->r_hint || !out->r_log_term ||
      !out->disposition || !out->deferred || !out->deferred_count)
    return QE_EINVAL;
  if (p->num_groups && !scratch) return QE_EINVAL;
  if (!al(scratch, 8)) return QE_EINVAL;
  if (n > 0xFFFFFFF0ull) return QE_ERANGE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0)
    return hip_status(hipMemsetAsync(out->deferred_count, 0, sizeof(uint64_t), st));
  IBArgs a{};
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.n = n;
  a.S = p->num_slots;
  a.E = in->msg_runs;
  a.fterm = f->term;
  a.fstate = f->state;
  a.group = in->group;
  a.from = in->from;
  a.type = in->type;
  a.term = in->term;
  a.index = in->index;
  a.log_term = in->log_term;
  a.commit = in->commit;
  a.hint = in->hint;
  a.ctx = in->ctx;
  a.flags = in->flags;
  a.ent_len = in->ent_len;
  a.ent_term = in->ent_term;
  a.tick = in->tick_action;
  a.f_type = out->f_type;
  a.f_from = out->f_from;
  a.f_term = out->f_term;
  a.f_index = out->f_index;
  a.f_log_term = out->f_log_term;
  a.f_commit = out->f_commit;
  a.f_ent_len = out->f_ent_len;
  a.f_ent_term = out->f_ent_term;
  a.s_type = out->s_type;
  a.s_from = out->s_from;
  a.s_term = out->s_term;
  a.s_snap_index = out->s_snap_index;
  a.s_snap_term = out->s_snap_term;
  a.v_type = out->v_type;
  a.v_from = out->v_from;
  a.v_term = out->v_term;
  a.v_index = out->v_index;
  a.v_log_term = out->v_log_term;
  a.v_flags = out->v_flags;
  a.r_type = out->r_type;
  a.r_index = out->r_index;
  a.r_hint = out->r_hint;
  a.r_log_term = out->r_log_term;
  a.r_ctx = out->r_ctx;
  a.f_src = out->f_src;
  a.s_src = out->s_src;
  a.v_src = out->v_src;
  a.r_src = out->r_src;
  a.disposition = out->disposition;
  a.stats = stats;
  ScanScratch sc;
  inbox_scratch(scratch, a, sc);  // (n is in range: its chunks fit a launch)
  int s = dispatch_inbox_init(a, st);
  if (s) return s;
  if (n) {
    s = dispatch_inbox_passes(a, st);
    if (s) return s;
    launch_count(a.dflag, n, sc, st);
  }
  s = launch_scan(sc, out->deferred_count, st);
  if (s || !n) return s;
  return dispatch_route_positions({n, sc.nb, sc.offsets, a.dflag, out->deferred}, st);
}

size_t qe_requests_scratch_bytes(uint64_t num_groups, uint64_t num_records) {
  RQArgs a{num_groups, 0, 0, num_records};  // (G, goff, stride, n)
  ScanScratch sd, so;
  return requests_scratch(nullptr, a, sd, so);
}

int qe_requests(const qe_progress *p, const qe_follower *f, const qe_requests_in *in,
                const qe_requests_out *out, void *scratch, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!f || !in || !out || !f->term || !f->state || !f->lead || !p->self_slot) return QE_EINVAL;
  if (in->reserved || (in->flags & ~QE_REQ_NO_FORWARD)) return QE_EINVAL;
  if (p->num_groups && p->stride < p->num_groups) return QE_EINVAL;
  if (in->max_cc > QE_PROP_MAX_CC) return QE_EINVAL;
  if (in->max_cc &&
      (out->cc_stride < p->num_groups || !out->p_cc_count || !out->p_cc_pos || !out->p_cc_leave ||
       !out->p_cc_size || (in->cc_count && (!in->cc_pos || !in->cc_leave || !in->cc_size))))
    return QE_EINVAL;
  const uint64_t n = in->num_records;
  if (n && (!in->group || !in->type || !in->from || !in->term || !in->index || !in->key))
    return QE_EINVAL;
  if (!out->p_num_entries || !out->ri_request || !out->ri_key || !out->ri_from || !out->v_type ||
      !out->v_from || !out->v_term || !out->v_index || !out->v_log_term || !out->r_type ||
      !out->disposition || !out->deferred || !out->deferred_count || !out->count)
    return QE_EINVAL;
  if (out->capacity && (!out->group || !out->kind || !out->type || !out->to || !out->from ||
                        !out->term || !out->index || !out->key || !out->src))
    return QE_EINVAL;
  if (p->num_groups && !scratch) return QE_EINVAL;
  if (!al(scratch, 8)) return QE_EINVAL;
  if (n > 0xFFFFFFF0ull) return QE_ERANGE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p->num_groups == 0) {
    const int s = hip_status(hipMemsetAsync(out->deferred_count, 0, sizeof(uint64_t), st));
    return s ? s : hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
  }
  RQArgs a{};
  a.G = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.n = n;
  a.cc_stride = out->cc_stride;
  a.S = p->num_slots;
  a.max_cc = in->max_cc;
  a.flags = in->flags;
  a.fterm = f->term;
  a.fstate = f->state;
  a.flead = f->lead;
  a.group = in->group;
  a.type = in->type;
  a.from = in->from;
  a.term = in->term;
  a.key = in->key;
  a.num_entries = in->num_entries;
  a.payload = in->payload;
  a.cc_count = in->cc_count;
  a.cc_pos = in->cc_count ? in->cc_pos : nullptr;
  a.cc_leave = in->cc_count ? in->cc_leave : nullptr;
  a.cc_size = in->cc_count ? in->cc_size : nullptr;
  a.p_num_entries = out->p_num_entries;
  a.p_payload = out->p_payload;
  a.p_cc_count = out->p_cc_count;
  a.p_cc_pos = out->p_cc_pos;
  a.p_cc_leave = out->p_cc_leave;
  a.p_cc_size = out->p_cc_size;
  a.ri_request = out->ri_request;
  a.ri_key = out->ri_key;
  a.ri_from = out->ri_from;
  a.v_type = out->v_type;
  a.v_from = out->v_from;
  a.v_term = out->v_term;
  a.v_index = out->v_index;
  a.v_log_term = out->v_log_term;
  a.v_flags = out->v_flags;
  a.r_type = out->r_type;
  a.p_src = out->p_src;
  a.ri_src = out->ri_src;
  a.v_src = out->v_src;
  a.r_src = out->r_src;
  a.disposition = out->disposition;
  a.stats = stats;
  ScanScratch sd, so;
  requests_scratch(scratch, a, sd, so);  // (n is in range: its chunks fit a launch)
  int s = dispatch_requests_init(a, st);
  if (s) return s;
  if (n) {
    s = dispatch_requests_passes(a, st);
    if (s) return s;
    launch_count(a.dflag, n, sd, st);
    launch_count(a.okind, n, so, st);
  }
  s = launch_scan(sd, out->deferred_count, st);
  if (s) return s;
  s = launch_scan(so, out->count, st);
  if (s || !n) return s;
  RQList l{};
  l.G = n;
  l.nb = so.nb;
  l.goff = p->group_offset;
  l.offsets = so.offsets;
  l.flag = a.okind;
  l.fterm = f->term;
  l.flead = f->lead;
  l.self_slot = p->self_slot;
  l.S = p->num_slots;
  l.group = in->group;
  l.type = in->type;
  l.from = in->from;
  l.index = in->index;
  l.key = in->key;
  l.cap = out->capacity;
  l.o_group = out->group;
  l.o_kind = out->kind;
  l.o_type = out->type;
  l.o_to = out->to;
  l.o_from = out->from;
  l.o_term = out->term;
  l.o_index = out->index;
  l.o_key = out->key;
  l.o_src = out->src;
  s = dispatch_requests_out(l, st);
  if (s) return s;
  return dispatch_route_positions({n, sd.nb, sd.offsets, a.dflag, out->deferred}, st);
}

size_t qe_carry_scratch_bytes(uint64_t capacity) {
  CRArgs a{capacity};  // (G: the source's capacity)
  ScanScratch sl, sr;
  return carry_scratch(nullptr, a, sl, sr);
}

int qe_carry(const qe_progress *p, const qe_peers *peers, const qe_carry_in *in,
             const qe_carry_out *out, void *scratch, uint64_t *stats, void *stream) {
  const int rc = check_progress(p);
  if (rc) return rc;
  if (!peers || !in || !out || !peers->peer_group || !peers->peer_from) return QE_EINVAL;
  if (in->reserved || out->reserved || (in->flags & ~QE_CARRY_SNAP_STATUS) ||
      (in->ignore & ~QE_CARRY_TYPES))
    return QE_EINVAL;
  if (p->num_groups && p->stride < p->num_groups) return QE_EINVAL;
  if (in->msg_runs > out->msg_runs || out->msg_runs > QE_MAX_MSG_RUNS) return QE_EINVAL;
  if (!in->count || !out->count || !out->remote_count) return QE_EINVAL;
  const uint64_t cap = in->capacity;
  if (cap && (!in->group || !in->to || !in->type || !in->term || !in->index || !in->log_term ||
              !out->disposition || !out->remote || !scratch))
    return QE_EINVAL;
  if (in->msg_runs && (!in->ent_len || !in->ent_term)) return QE_EINVAL;
  if (out->base > out->capacity) return QE_EINVAL;
  if (out->capacity &&
      (!out->group || !out->from || !out->type || !out->term || !out->index || !out->log_term ||
       !out->commit || !out->hint ||
       (out->msg_runs && (!out->ent_len || !out->ent_term || out->ent_pitch < out->capacity))))
    return QE_EINVAL;
  if (!al(scratch, 8)) return QE_EINVAL;
  if (cap > 0xFFFFFFF0ull) return QE_ERANGE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (cap == 0) {
    const int s = hip_status(hipMemsetAsync(out->count, 0, sizeof(uint64_t), st));
    return s ? s : hip_status(hipMemsetAsync(out->remote_count, 0, sizeof(uint64_t), st));
  }
  CRArgs a{};
  a.G = cap;
  a.ng = p->num_groups;
  a.goff = p->group_offset;
  a.stride = p->stride;
  a.S = p->num_slots;
  a.E_in = in->msg_runs;
  a.E_out = out->msg_runs;
  a.flags = in->flags;
  a.ignore = in->ignore;
  a.cut_wide = p->num_slots > 8;
  a.peer_group = peers->peer_group;
  a.peer_from = peers->peer_from;
  a.icount = in->count;
  a.group = in->group;
  a.to = in->to;
  a.type = in->type;
  a.term = in->term;
  a.index = in->index;
  a.log_term = in->log_term;
  a.commit = in->commit;
  a.hint = in->hint;
  a.ctx = in->ctx;
  a.mflags = in->mflags;
  a.ent_len = in->ent_len;
  a.ent_term = in->ent_term;
  a.drop = in->drop;
  a.cut = in->cut;
  a.ocap = out->capacity;
  a.base = out->base;
  a.pitch = out->ent_pitch;
  a.o_group = out->group;
  a.o_from = out->from;
  a.o_type = out->type;
  a.o_term = out->term;
  a.o_index = out->index;
  a.o_log_term = out->log_term;
  a.o_commit = out->commit;
  a.o_hint = out->hint;
  a.o_ctx = out->ctx;
  a.o_mflags = out->mflags;
  a.o_ent_len = out->ent_len;
  a.o_ent_term = out->ent_term;
  a.o_src = out->src;
  a.disposition = out->disposition;
  a.stats = stats;
  ScanScratch sl, sr;
  carry_scratch(scratch, a, sl, sr);  // (cap is in range: its chunks fit a launch)
  int s = dispatch_carry_classify(a, st);
  if (s) return s;
  s = dispatch_carry_count(a, st);
  if (s) return s;
  launch_count(a.rflag, cap, sr, st);
  s = launch_scan(sl, out->count, st);
  if (s) return s;
  s = launch_scan(sr, out->remote_count, st);
  if (s) return s;
  s = dispatch_carry_fill(a, st);
  if (s) return s;
  return dispatch_route_positions({cap, sr.nb, sr.offsets, a.rflag, out->remote}, st);
}

int qe_stats_reduce(const uint64_t *stats, uint64_t *out, void *stream) {
  if (!stats || !out) return QE_EINVAL;
  hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     stats, out);
  return hip_status(hipGetLastError());
}

int qe_gen_groups(const qe_groups *g, const qe_gen_params *p, void *stream) {
  int rc = check_groups(g);
  if (rc) return rc;
  if (!p) return QE_EINVAL;
  if (g->num_groups == 0) return QE_OK;
  if (p->p_absent_q16 > 65536 || p->p_voted_q16 > 65536 || p->p_granted_q16 > 65536)
    return QE_ERANGE;
  GArgs a{};
  a.G = g->num_groups;
  a.goff = g->group_offset;
  a.stride = g->stride;
  a.S = g->num_slots;
  a.match = const_cast<uint64_t *>(g->match);
  a.inc = const_cast<void *>(g->inc_mask);
  a.out = const_cast<void *>(g->out_mask);
  a.learner = const_cast<void *>(g->learner_mask);
  a.voted = const_cast<void *>(g->voted);
  a.granted = const_cast<void *>(g->granted);
  a.p = *p;
  // qe_gen_params.group_offset adds to qe_groups.group_offset.
  a.goff = g->group_offset + p->group_offset;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = elem_grid(g->num_groups, num_cus());
  if (g->num_slots <= 8)
    hipLaunchKernelGGL(k_gen<uint8_t>, dim3(grid), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(k_gen<uint16_t>, dim3(grid), dim3(kBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // extern "C"
