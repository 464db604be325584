/*
 * etcd_quorum.h — C ABI of the MI355X batched Raft quorum engine.
 *
 * This is the drop-in boundary for etcd's raft/quorum + raft/tracker hot path
 * (reference: /root/reference/raft, etcd 3.6.0-pre).  The per-group Go API
 * (MajorityConfig / JointConfig / ProgressTracker) stays the semantic
 * reference; every entry point below evaluates the same decision for G
 * independent Raft groups in one call on the GPU.  See INTEGRATION.md for the
 * cgo binding a maintainer adds next to raft/quorum.
 *
 * Data model ("slot SoA")
 *   A group's peers (voters of both halves, learners) are packed into S <= 16
 *   slots.  Slot order is arbitrary: every function here is an order-free set
 *   function of the (voter set, per-voter value) pairs, exactly like the Go
 *   code which iterates maps (raft/quorum/majority.go:155-161 fills then sorts).
 *
 *   match    uint64 [S][stride]   Progress.Match per slot; "absent" (no acked
 *                                 index, AckedIndexer.found == false) is 0,
 *                                 which CommittedIndex treats identically
 *                                 (raft/quorum/majority.go:150-161).
 *   masks    per-group slot bitmaps; element type is uint8_t when S <= 8 and
 *            uint16_t when 9 <= S <= 16 (qe_mask_bytes(S)).
 *            inc_mask  = JointConfig[0] (incoming voters)
 *            out_mask  = JointConfig[1] (outgoing voters; NULL = not joint)
 *            learner_mask = tracker.Config.Learners (optional)
 *            voted / granted = ProgressTracker.Votes: bit s of voted set iff
 *            slot s has a recorded vote, bit s of granted = that vote's value.
 *            A NULL inc_mask means "all S slots are voters" (fixed-size
 *            MajorityConfig, the BenchmarkMajorityConfig_CommittedIndex shape).
 *
 * Conventions
 *   - Index infinity (math.MaxUint64, raft/quorum/quorum.go:25-30) is
 *     QE_INDEX_INF.
 *   - VoteResult uses the reference's numeric encoding
 *     VotePending=1, VoteLost=2, VoteWon=3 (raft/quorum/quorum.go:48-58).
 *   - All pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) unless
 *     the parameter says host.  The library allocates nothing and retains
 *     nothing; `stream` is a hipStream_t (NULL = default stream).  Calls are
 *     asynchronous on `stream` and reentrant on distinct buffers.
 *   - Return value: QE_OK or a negative QE_E* code.  num_groups == 0 is a
 *     successful no-op.  Semantic "panics" of the reference become counters
 *     in the optional stats buffer, never aborts.
 *   - Alignment: match/next/commit arrays 16-byte aligned and stride even
 *     take the vectorised path; anything else is still correct (scalar path).
 */
#ifndef ETCD_QUORUM_H
#define ETCD_QUORUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QE_ABI_VERSION 8  /* 8: see INTEGRATION.md "ABI 8" (changes listed there) */

#define QE_INDEX_INF UINT64_MAX
#define QE_MAX_SLOTS 16

/* quorum.VoteResult (raft/quorum/quorum.go:48-58) */
#define QE_VOTE_PENDING 1
#define QE_VOTE_LOST 2
#define QE_VOTE_WON 3

/* Raft StateType subset used by the election simulation (raft/raft.go:
 * StateFollower=0, StateCandidate=1, StateLeader=2, StatePreCandidate=3). */
#define QE_STATE_FOLLOWER 0
#define QE_STATE_CANDIDATE 1
#define QE_STATE_LEADER 2
#define QE_STATE_PRE_CANDIDATE 3

/* Status codes */
#define QE_OK 0
#define QE_EINVAL (-22)  /* null pointer / bad size / S out of range   */
#define QE_ERANGE (-34)  /* value out of supported range                */
#define QE_EHIP (-1000)  /* HIP launch / runtime error                  */
#define QE_ECOMM (-1001) /* RCCL error (qe_comm_*, qe_allreduce_stats)    */

/* Aggregate statistics.  A stats buffer is uint64[QE_STATS_WORDS]; kernels
 * add into QE_STATS_SHARDS shards of QE_STATS_COUNTERS counters (one 128-byte
 * line per shard) to avoid a single hot atomic line.  qe_stats_reduce() folds
 * the shards.  Counters accumulate across calls until the caller zeroes the
 * buffer, so one all-reduce at the end of a run aggregates a whole job. */
#define QE_STATS_COUNTERS 16
#define QE_STATS_SHARDS 64
#define QE_STATS_WORDS (QE_STATS_COUNTERS * QE_STATS_SHARDS)
enum qe_stat {
  QE_STAT_GROUPS = 0,        /* groups evaluated                              */
  QE_STAT_COMMIT_INF = 1,    /* CommittedIndex == inf (empty config)          */
  QE_STAT_COMMIT_SUM = 2,    /* sum of finite committed indexes (mod 2^64)    */
  QE_STAT_COMMIT_ZERO = 3,   /* CommittedIndex == 0 (nothing committed)       */
  QE_STAT_VOTE_WON = 4,
  QE_STAT_VOTE_LOST = 5,
  QE_STAT_VOTE_PENDING = 6,
  QE_STAT_GRANTED = 7,       /* sum of TallyVotes granted                      */
  QE_STAT_REJECTED = 8,      /* sum of TallyVotes rejected                     */
  QE_STAT_COMMIT_ADVANCED = 9,   /* replication: commit advanced this round    */
  QE_STAT_READ_RELEASED = 10,    /* ReadIndex requests released (a request count,
                                    * not groups; replication: quorum reached)  */
  QE_STAT_ELECTIONS = 11,        /* election sim: campaigns started            */
  QE_STAT_LEADERS = 12,          /* election sim: elections won                */
  QE_STAT_STEPDOWNS = 13,        /* election sim: elections lost               */
  QE_STAT_INVARIANT_VIOLATIONS = 14, /* learner∩voter≠∅, mci>lastIndex, ...  */
  QE_STAT_CHECKSUM = 15          /* mixed hash of all outputs (order-free)     */
};

/* A batch of G groups in slot-SoA form (see header comment). */
typedef struct qe_groups {
  uint64_t num_groups;       /* G                                            */
  uint64_t group_offset;     /* global id of group 0 (checksum key; shards)  */
  uint32_t num_slots;        /* S, 1..16                                     */
  uint32_t reserved;         /* must be 0                                    */
  uint64_t stride;           /* elements between slot rows of match (>= G)   */
  const uint64_t *match;     /* [S][stride] acked index per slot, 0 = absent */
  const void *inc_mask;      /* [G] JointConfig[0]; NULL = all S slots       */
  const void *out_mask;      /* [G] JointConfig[1]; NULL = non-joint         */
  const void *learner_mask;  /* [G] Learners; NULL = none                    */
  const void *voted;         /* [G] vote recorded bitmap; NULL = no votes    */
  const void *granted;       /* [G] vote value bitmap; NULL = all "no"       */
} qe_groups;

/* Outputs of the fused evaluation.  Any pointer may be NULL to skip it. */
typedef struct qe_outputs {
  uint64_t *commit;          /* [G] JointConfig.CommittedIndex               */
  uint8_t *vote;             /* [G] JointConfig.VoteResult (1/2/3)           */
  uint8_t *granted_count;    /* [G] TallyVotes granted                       */
  uint8_t *rejected_count;   /* [G] TallyVotes rejected                      */
  uint64_t *stats;           /* uint64[QE_STATS_WORDS] accumulated, or NULL  */
} qe_outputs;

/* ---- introspection ---------------------------------------------------- */
int qe_abi_version(void);
const char *qe_strerror(int status);
size_t qe_mask_bytes(uint32_t num_slots); /* 1 for S<=8, 2 for S<=16, 0 bad */

/* Optional launch tuning (no reference counterpart; never changes results):
 *   "blocks_per_cu"  cap on persistent-grid workgroups per CU, 0..32
 *                    (default 0 = the kernel's occupancy)
 *   "tiles_per_wave" -1 = per-kernel default (measured best), 0 =
 *                    persistent grid, T > 0: each wave walks T tiles
 *   "nontemporal"    bit 0: non-temporal loads, bit 1: non-temporal stores
 *                    of qe_commit_vote                                     */
int qe_tune(const char *key, int value);

/* ---- quorum decisions -------------------------------------------------- */

/* Fused ProgressTracker.Committed + TallyVotes for every group:
 *   commit[g] = Voters.CommittedIndex(match)           tracker.go:177-179,
 *               joint.go:49-56, majority.go:126-172
 *   vote[g]   = Voters.VoteResult(votes)               tracker.go:286,
 *               joint.go:61-75, majority.go:178-210
 *   granted/rejected_count[g] = TallyVotes counts over non-learner voters
 *               tracker.go:267-285
 * Replaces one AckedIndexer-driven CommittedIndex call plus one
 * VoteResult(map) call per group (raft/quorum/majority.go:126, :178). */
int qe_commit_vote(const qe_groups *groups, const qe_outputs *out,
                   void *stream);

/* JointConfig.CommittedIndex only (MajorityConfig when out_mask == NULL).
 * raft/quorum/joint.go:49-56, raft/quorum/majority.go:126-172. */
int qe_committed_index(const qe_groups *groups, uint64_t *commit,
                       void *stream);

/* JointConfig.VoteResult only; `voted`/`granted` give the votes map.
 * raft/quorum/joint.go:61-75, raft/quorum/majority.go:178-210. */
int qe_vote_result(const qe_groups *groups, uint8_t *vote, void *stream);

/* ProgressTracker.QuorumActive (raft/tracker/tracker.go:215-225): every
 * non-learner voter votes Progress.RecentActive; active[g] = 1 iff the
 * result is VoteWon.  `recent_active` is a [G] slot bitmap (mask type). */
int qe_quorum_active(const qe_groups *groups, const void *recent_active,
                     uint8_t *active, void *stream);

/* ProgressTracker.RecordVote (raft/tracker/tracker.go:258-263) for a batch of
 * vote responses: for each group, slots in `resp_mask` cast vote
 * `resp_value`; the first recorded vote per slot sticks.  Updates
 * voted/granted in place (mask-typed [G] arrays). */
int qe_record_votes(uint64_t num_groups, uint32_t num_slots, void *voted,
                    void *granted, const void *resp_mask,
                    const void *resp_value, void *stream);

/* ---- lockstep replication round (BASELINE config 4) -------------------- */

/* Device-resident leader-side state of G groups. */
typedef struct qe_repl_state {
  uint64_t num_groups;
  uint64_t group_offset;     /* global id of group 0 (checksum key)          */
  uint32_t num_slots;
  uint32_t reserved;
  uint64_t stride;           /* slot-row stride of match/next               */
  uint64_t *match;           /* [S][stride] Progress.Match (rw)             */
  uint64_t *next;            /* [S][stride] Progress.Next  (rw)             */
  uint64_t *committed;       /* [G] raftLog.committed (rw)                  */
  const uint64_t *term_start;/* [G] first index of the leader's term         */
  const uint64_t *last_index;/* [G] raftLog.lastIndex()                      */
  const void *inc_mask;      /* [G] as in qe_groups                          */
  const void *out_mask;      /* [G] or NULL                                  */
} qe_repl_state;

/* One round of MsgAppResp / MsgHeartbeatResp handling per group. */
typedef struct qe_repl_msgs {
  const uint64_t *resp_index;/* [S][stride] MsgAppResp.Index per slot        */
  const void *resp_mask;     /* [G] slots whose (non-reject) MsgAppResp came */
  const void *read_acks;     /* [G] ReadIndex heartbeat acks (incl. self), or NULL */
  uint8_t *read_ok;          /* [G] out: VoteResult(acks)==VoteWon, or NULL */
  uint8_t *commit_advanced;  /* [G] out: maybeCommit() returned true, or NULL */
} qe_repl_msgs;

/* For each group: Progress.MaybeUpdate(resp) on every responding slot
 * (raft/tracker/progress.go:144-153), then raft.maybeCommit
 * (raft/raft.go:585-588 -> raft/log.go:325-331 -> commitTo log.go:233-241)
 * with the synthetic log model term(i)==Term <=> term_start<=i<=last_index,
 * then the ReadIndex quorum check VoteResult(acks)==VoteWon
 * (raft/raft.go:1300, raft/read_only.go:68-76). */
int qe_replication_round(const qe_repl_state *st, const qe_repl_msgs *msgs,
                         uint64_t *stats, void *stream);

/* ---- randomized election simulation (BASELINE config 5) ---------------- */

typedef struct qe_election_state {
  uint64_t num_groups;
  uint64_t group_offset;     /* global id of group 0 (RNG key; sharding)     */
  uint32_t num_slots;
  uint32_t reserved;
  uint64_t *term;            /* [G] rw                                       */
  uint8_t *state;            /* [G] rw QE_STATE_*                            */
  void *voted;               /* [G] rw mask-typed                            */
  void *granted;             /* [G] rw mask-typed                            */
  const uint8_t *self_slot;  /* [G] candidate's own slot                     */
  const void *inc_mask;      /* [G]                                          */
  const void *out_mask;      /* [G] or NULL                                  */
  const void *learner_mask;  /* [G] or NULL (learners vote; never counted)   */
} qe_election_state;

typedef struct qe_election_params {
  uint64_t seed;
  uint64_t step0;            /* global step number of the first step         */
  uint32_t steps;            /* fused steps per launch (state in registers)  */
  uint32_t p_drop_q16;       /* P(response dropped) * 65536                  */
  uint32_t p_grant_q16;      /* P(vote granted | delivered) * 65536          */
  uint32_t flags;            /* QE_ELEC_* (ABI 1: reserved, 0)                */
  uint32_t p_active_q16;     /* CheckQuorum: P(a leader heard from a peer
                                within an election timeout) * 65536        */
  uint32_t reserved;
  /* Scripted mode (replaying a recorded or test message flow): when
   * script_resp is non-NULL, step k of group g takes its responses from
   * [k*script_stride + g] of these arrays instead of the RNG. */
  const void *script_resp;   /* mask-typed: peers whose (pre)vote response
                                arrives / that were active (CheckQuorum)   */
  const void *script_grant;  /* mask-typed: the responses that grant        */
  const uint8_t *script_hup; /* 1: the election timeout fires this step
                                (a (pre)candidate campaigns again); NULL
                                = never                                     */
  uint64_t script_stride;    /* >= num_groups                                */
} qe_election_params;

#define QE_ELEC_PREVOTE 1u       /* raft.Config.PreVote                      */
#define QE_ELEC_CHECK_QUORUM 2u  /* raft.Config.CheckQuorum                  */

/* `steps` election steps per group:
 *   Leader: CheckQuorum on -> one CheckQuorum round (raft/raft.go:997-1018):
 *     the leader sees itself active, each other voter active with
 *     p_active; !QuorumActive (tracker.go:215-225) -> becomeFollower (term
 *     kept).  CheckQuorum off -> the leader is deposed and campaigns.
 *   Follower (or a (pre)candidate whose timeout fires, script_hup): hup ->
 *     campaign (raft.go:785-803): PreVote on -> becomePreCandidate (term
 *     kept), else becomeCandidate (term+1); self-vote; a won tally moves on
 *     (pre-vote -> election -> leader).
 *   PreCandidate / Candidate: one round of responses from every other voter
 *     (drops/grants from a counter-based RNG) -> RecordVote -> TallyVotes
 *     (raft.go:837-845, :1399-1414): won -> campaign(campaignElection) /
 *     becomeLeader; lost -> becomeFollower (term kept); pending -> stay.
 * Invariant checks go to stats. */
int qe_election_steps(const qe_election_state *st,
                      const qe_election_params *p, uint64_t *stats,
                      void *stream);

/* ---- Progress state machine ------------------ */

/* tracker.StateType (raft/tracker/state.go) and the packed per-peer word
 * (ABI 3: one u32 per peer replaces the flags / Inflights.start /
 * Inflights.count byte rows of ABI 2, so a peer's small fields move in one
 * 4-byte access; ABI 4 adds the ring representation bits):
 *   bits 0-1   StateType (QE_PR_*)          bit 2  Progress.ProbeSent
 *   bit 3      Progress.RecentActive        bit 4  QE_PF_RING_WIDE
 *   bits 5-7   ring epoch bits 0-2          bits 8-15  Inflights.start
 *   bits 16-23 Inflights.count              bits 24-31 ring epoch bits 3-10
 * Inflights entries are stored as 32-bit words (infl_lo); the upper 32 bits
 * of an entry are the peer's 11-bit ring epoch H (QE_PW_EPOCH) unless
 * QE_PF_RING_WIDE is set, in which case they are infl_hi's word:
 *   entry k = ((wide ? infl_hi[k] : H) << 32) | infl_lo[k].
 * The form is canonical when count == 0 -> H = 0, not wide; else not wide
 * iff every live entry's upper word is the same value < 2^11 (entries below
 * 2^43 within one 2^32-aligned window: every realistic in-flight window),
 * which is then H.  qe_ring_pack produces it and the kernels restore it
 * whenever they append (a ring they only free entries from may stay wide).
 * qe_ring_pack / qe_ring_unpack convert plain uint64 rings.  Ring
 * representation bits are not Progress state: QE_PW_RING_MASK selects them.
 *
 * ABI 8, the 16-bit form (qe_progress.infl16 non-NULL; F <= QE_RING16_MAX_F):
 * the rings live in infl16 [S][stride][8] as offsets below Next,
 *   entry k = Progress.Next - 1 - infl16[k]        (not wide)
 *   entry k = (infl_hi[k] << 32) | infl_lo[k]       (QE_PF_RING_WIDE)
 * -- 16 bytes per peer, two peers per 32-byte HBM sector.  Live Inflights
 * entries are the last indices of MsgApps sent, all below Next; Next moves
 * only when an append rewrites the ring (OptimisticUpdate), or when the ring
 * empties (MaybeUpdate past every sent index, ResetState).  A peer is wide
 * iff some live entry lies outside [Next - 65536, Next - 1] (a window of
 * more than 65536 indices, or an inconsistent input); the epoch bits are 0.
 * The kernels re-encode a peer's ring whenever they append to it or change
 * its Next while entries are live.  Entry points that write Next without
 * knowing the rings (qe_apply_append_resps, a host) must not be used on the
 * Next rows of such a state while entries are live: they would re-base the
 * entries.  qe_ring_pack16 / qe_ring_unpack16 convert plain uint64 rings. */
#define QE_PR_PROBE 0
#define QE_PR_REPLICATE 1
#define QE_PR_SNAPSHOT 2
#define QE_PF_STATE 3u          /* word & QE_PF_STATE = StateType            */
#define QE_PF_PROBE_SENT 4u     /* Progress.ProbeSent                        */
#define QE_PF_RECENT_ACTIVE 8u  /* Progress.RecentActive                     */
#define QE_PF_RING_WIDE 16u     /* ABI 4: entries' upper words in infl_hi     */
#define QE_PW_START_SHIFT 8     /* Inflights.start = (word >> 8) & 0xFF       */
#define QE_PW_COUNT_SHIFT 16    /* Inflights.count = (word >> 16) & 0xFF      */
#define QE_PW_RING_MASK 0xFF0000F0u /* ABI 4: WIDE + epoch bits               */
#define QE_RING_EPOCH_MAX 0x7FFu    /* largest epoch held in the word         */
#define QE_PW_EPOCH(w) ((((w) >> 5) & 7u) | (((w) >> 21) & 0x7F8u))
#define QE_PW_EPOCH_BITS(h) ((((uint32_t)(h) & 7u) << 5) | (((uint32_t)(h) & 0x7F8u) << 21))
#define QE_PW_PACK(state, probe_sent, recent_active, start, count)                 \
  ((uint32_t)(state) | ((probe_sent) ? QE_PF_PROBE_SENT : 0u) |                   \
   ((recent_active) ? QE_PF_RECENT_ACTIVE : 0u) |                                 \
   ((uint32_t)(start) << QE_PW_START_SHIFT) | ((uint32_t)(count) << QE_PW_COUNT_SHIFT))
/* ABI 4: words per peer ring in infl_lo / infl_hi (F rounded up to 4, so a
 * ring of F <= 8 is one or two 16-byte accesses, one 32-byte HBM sector) */
#define QE_RING_PITCH(F) (((uint32_t)(F) + 3u) & ~3u)
#define QE_MAX_INFLIGHT 255     /* Inflights capacity (MaxInflightMsgs)      */
#define QE_RING16_MAX_F 8       /* ABI 8: the 16-bit form holds up to 8 entries */
#define QE_RING16_MAX_SLOTS 9   /* ABI 8: ... for up to 9 slots (the pipelined
                                   Progress kernels' shapes) and log_runs <= 4 */
#define QE_MAX_LOG_RUNS 16      /* term runs of the leader-log model          */

/* message kinds of qe_peer_msgs.type (any other value: no message) */
#define QE_MSG_NONE 0
#define QE_MSG_APP_RESP 1             /* MsgAppResp, Reject=false            */
#define QE_MSG_APP_RESP_REJECT 2      /* MsgAppResp, Reject=true             */
#define QE_MSG_HEARTBEAT_RESP 3       /* MsgHeartbeatResp                    */
#define QE_MSG_SNAP_STATUS 4          /* MsgSnapStatus, Reject=false         */
#define QE_MSG_SNAP_STATUS_REJECT 5   /* MsgSnapStatus, Reject=true          */
#define QE_MSG_UNREACHABLE 6          /* MsgUnreachable                      */
#define QE_MSG_TRANSFER_LEADER 7      /* ABI 5: MsgTransferLeader, m.From = the
                                         slot (raft.go:1339-1370)            */

/* ABI 5: ReadIndex requests a leader keeps pending under ReadOnlySafe
 * (readOnly.pendingReadIndex + readIndexQueue, raft/read_only.go:39-63).
 * Each request has a context number (the engine's stand-in for the
 * request's context bytes, unique within the group): queue entry j has
 * context read_head + j; numbers are 32-bit, assigned consecutively by
 * qe_read_index, never 0 (0 = no context).  The first QE_READ_QUEUE entries
 * live in one word per group (read_acks, the fast form every kernel reads
 * with the group); ABI 7: a queue of up to read_cap entries keeps entries
 * QE_READ_QUEUE.. in the overflow ring read_ovf, each at its context number
 * mod read_cap (an entry never moves while it waits there). */
#define QE_READ_QUEUE 4
#define QE_READ_CAP_MAX 255     /* read_count is a byte                      */

/* Leader-side Progress of every peer of G groups (raft/tracker/progress.go:
 * 30-80) plus the leader's log model: term runs r < run_count[g] covering
 * [run_first[r], run_first[r+1]) with run_term[r] (run 0 starts at the
 * snapshot/dummy index = first_index - 1), ending at last_index; the current
 * term's entries are [term_start, last_index].  Entries exist in
 * [first_index, last_index]; max_ents models MaxSizePerMsg for equal-size
 * entries (entries per MsgApp, at least one; 0 = noLimit).  Inflights.start
 * must be < inflight_cap (results are unspecified otherwise; memory stays in
 * bounds). */
typedef struct qe_progress {
  uint64_t num_groups;
  uint64_t group_offset;
  uint32_t num_slots;
  uint32_t inflight_cap;        /* F = MaxInflightMsgs, 1..QE_MAX_INFLIGHT  */
  uint64_t stride;
  uint64_t *match, *next;       /* [S][stride]                               */
  uint64_t *pending_snapshot;   /* [S][stride]; 0 for a peer not in
                                 * StateSnapshot (every reachable Progress:
                                 * ResetState clears it on each state change,
                                 * tracker/progress.go:84-89) -- the kernels
                                 * write it only where its value changes      */
  uint32_t *peer;               /* [S][stride] packed per-peer word (ABI 3):
                                   StateType, ProbeSent, RecentActive,
                                   Inflights.start / count (QE_PW_*)         */
  uint32_t *infl_lo;            /* ABI 4: [S][stride][QE_RING_PITCH(F)]
                                   Inflights.buffer, low 32 bits, lane-major:
                                   entry k of slot s of group g at
                                   (s*stride + g)*QE_RING_PITCH(F) + k       */
  uint32_t *infl_hi;            /* ABI 4: same shape, high 32 bits; read and
                                   written only for QE_PF_RING_WIDE peers    */
  uint64_t *committed;          /* [G] raftLog.committed (rw)                */
  const uint64_t *term_start;   /* [G]                                       */
  const uint64_t *first_index;  /* [G] raftLog.firstIndex()                  */
  const uint64_t *last_index;   /* [G] raftLog.lastIndex()                   */
  uint32_t log_runs;            /* R <= QE_MAX_LOG_RUNS                      */
  uint32_t reserved;
  const uint64_t *run_first;    /* [R][stride]                               */
  const uint64_t *run_term;     /* [R][stride]                               */
  const uint8_t *run_count;     /* [G] valid runs, 1..R                       */
  const void *inc_mask;         /* [G] as in qe_groups (NULL = all slots)    */
  const void *out_mask;         /* [G] or NULL                               */
  /* ABI 2 */
  const void *tracked;          /* [G] slots holding a Progress (ProgressMap
                                   keys); NULL = every slot                  */
  const uint8_t *self_slot;     /* [G] the leader's own slot (bcastAppend
                                   skips it); NULL or >= S = none            */
  uint8_t *lead_transferee;     /* [G] rw (ABI 5): slot of r.leadTransferee;
                                   >= S = no transfer in progress (None).
                                   MsgTransferLeader rewrites it; NULL = no
                                   transfer in progress and the round's
                                   changes are not stored                    */
  const uint64_t *snap_index;   /* [G] index of the snapshot a MsgSnap
                                   carries; NULL = first_index - 1           */
  uint32_t max_ents;            /* entries per MsgApp (0 = noLimit)          */
  uint32_t reserved2;
  /* ABI 5: the ReadIndex queue (r.readOnly, ReadOnlySafe); NULL read_acks =
   * no requests tracked (heartbeat contexts are ignored). */
  void *read_acks;              /* [G][QE_READ_QUEUE] rw mask-typed: acks of
                                   queue entry j (0 = oldest) of group g at
                                   read_acks[g*QE_READ_QUEUE + j] (one 4- or
                                   8-byte word per group)                    */
  uint32_t *read_head;          /* [G] rw: context number of queue entry 0   */
  uint8_t *read_count;          /* [G] rw: pending requests, 0..read_cap     */
  /* ABI 7: a queue longer than the word (readIndexQueue is unbounded in the
   * reference, read_only.go:56-63) and the duplicate-request check */
  uint32_t read_cap;            /* entries a queue holds: 0 (= QE_READ_QUEUE,
                                   ABI 5) or QE_READ_QUEUE..QE_READ_CAP_MAX  */
  uint32_t reserved3;           /* must be 0                                 */
  void *read_ovf;               /* [G][read_cap] rw mask-typed: the acks of
                                   the entry with context c at queue position
                                   >= QE_READ_QUEUE, at read_ovf[g*read_cap +
                                   c % read_cap]; needed when read_cap >
                                   QE_READ_QUEUE                             */
  uint64_t *read_keys;          /* [G][read_cap] rw: the caller's key (e.g. a
                                   hash of the request context bytes) of the
                                   entry with context c, at read_keys[g*
                                   read_cap + c % read_cap]; NULL = keys not
                                   tracked.  Given, it must have been given to
                                   every qe_read_index that queued the pending
                                   entries                                   */
  /* ABI 8 */
  uint16_t *infl16;             /* [S][stride][8] rw or NULL: the 16-bit
                                   Inflights form (see QE_RING16_MAX_F above;
                                   infl_lo / infl_hi then hold the wide peers
                                   only).  Requires inflight_cap <=
                                   QE_RING16_MAX_F, num_slots <=
                                   QE_RING16_MAX_SLOTS, log_runs <= 4        */
} qe_progress;

/* One round of peer responses: message of slot s for group g at
 * [s*stride + g].  Outputs may be NULL. */
typedef struct qe_peer_msgs {
  const uint8_t *type;          /* QE_MSG_*                                  */
  const uint64_t *index;        /* m.Index                                   */
  const uint64_t *reject_hint;  /* m.RejectHint                              */
  const uint64_t *log_term;     /* m.LogTerm                                 */
  void *sent;                   /* [G] out: slots sent >= 1 MsgApp/MsgSnap   */
  uint8_t *bcast;               /* [G] out: bcastAppend calls (commit advances) */
  void *snap;                   /* [G] out: slots sent a MsgSnap             */
  void *timeout_now;            /* [G] out: slots sent MsgTimeoutNow         */
  uint8_t *msg_count;           /* [S][stride] out: MsgApp/MsgSnap sent to the
                                   peer this round (saturates at 255)        */
  uint64_t *msg_index;          /* [S][stride] out: m.Index of the first of
                                   them (MsgSnap: the snapshot index);
                                   written only where msg_count > 0          */
  uint64_t *bytes_requested;    /* measurement aid, normally NULL: when set,
                                   an instrumented kernel adds the bytes the
                                   round reads and writes (field granularity,
                                   the rules of DESIGN.md §3) to
                                   *bytes_requested                          */
  /* ABI 5: ReadIndex under ReadOnlySafe against the queue of p
   * (raft.go:1296-1309, read_only.go:68-112) */
  const uint32_t *read_ctx;     /* [S][stride]: context number a
                                   MsgHeartbeatResp carries (0 = none,
                                   len(m.Context) == 0); NULL = every one
                                   carries the newest context pending when
                                   the round starts (bcastHeartbeat attaches
                                   lastPendingRequestCtx, raft.go:525-532)   */
  uint8_t *read_released;       /* [G] out (may be NULL): requests released
                                   this round, oldest first (readOnly.advance
                                   dequeues through the acked request)      */
  uint8_t *term_commit;         /* [G] out (may be NULL): 1 when this round's
                                   maybeCommit made committedEntryInCurrentTerm
                                   true, i.e. the leader's postponed
                                   MsgReadIndex requests are released now
                                   (raft.go:1259-1262, :1731-1733, :1813-1825) */
  uint64_t *term_commit_index;  /* [G] out (may be NULL): raftLog.committed
                                   right after that maybeCommit -- the index
                                   the released requests are added at
                                   (sendMsgReadIndexResponse, raft.go:1834);
                                   written only where term_commit is 1       */
} qe_peer_msgs;

/* Leader-side handling of one message per peer, slots in ascending order
 * (stepLeader, raft/raft.go:1099-1338), with every send the reference makes
 * while handling the message executed in place (max_ents from p):
 *   MsgAppResp reject: RecentActive; findConflictByTerm (raft/log.go:147-168)
 *     when LogTerm > 0; MaybeDecrTo (progress.go:170-193) -> Replicate ->
 *     BecomeProbe, sendAppend.
 *   MsgAppResp accept: RecentActive; IsPaused; MaybeUpdate -> Probe ->
 *     BecomeReplicate / Snapshot caught up -> BecomeProbe + BecomeReplicate /
 *     Replicate -> Inflights.FreeLE; maybeCommit -> bcastAppend (every tracked
 *     slot but self_slot) or sendAppend if it was paused; then
 *     `for maybeSendAppend(from, false) {}`; MsgTimeoutNow to the lead
 *     transferee once its Match == lastIndex (raft.go:1275-1281).
 *   MsgHeartbeatResp: RecentActive, ProbeSent = false, FreeFirstOne when the
 *     inflights are full, sendAppend if Match < lastIndex; with p->read_acks,
 *     a response carrying a context (ABI 5): recvAck on the queue entry with
 *     that context number (none pending: nothing is recorded), and once
 *     Voters.VoteResult(that entry's acks) == VoteWon, readOnly.advance
 *     releases every entry up to and including it (read_only.go:68-112).
 *   MsgSnapStatus (StateSnapshot only): reject -> PendingSnapshot = 0;
 *     BecomeProbe; ProbeSent = true (raft.go:1310-1331).
 *   MsgUnreachable: Replicate -> BecomeProbe (raft.go:1332-1338).
 *   MsgTransferLeader (ABI 5, raft.go:1339-1370): a learner's is ignored; a
 *     transfer to the slot already in progress is ignored; another transfer
 *     in progress is aborted; a transfer to self_slot is then ignored;
 *     otherwise lead_transferee = the slot, and MsgTimeoutNow goes out at
 *     once when its Match == lastIndex, else sendAppend to it.  (The
 *     reference also resets electionElapsed: tick state stays with the host,
 *     which sees the new lead_transferee and reports it to the next tick as
 *     QE_TEV_HEARD.)
 * A send is raft.maybeSendAppend (raft.go:432-492) on the log model; see
 * qe_progress_send.  Messages from untracked slots are dropped.  An accept
 * with index > lastIndex is processed as the reference does and counted as
 * an invariant violation.
 * The sends are reported as masks (sent, snap) and msg_index, not as messages.
 * Building MsgApp{Index, LogTerm, Entries, Commit} / MsgSnap from them used to
 * be a host duty for every leader-side entry point (walk the run table of the
 * group for every set bit); it is optional now: qe_outbox lists the messages
 * of one call's masks on the device.
 * qe_peer_msgs carries no term: raft.Step's preamble (raft.go:849-920) for
 * these messages is the HOST's (or qe_inbox's, which runs it on a list of
 * delivered messages and fills these rows).  Only a response of the group's own term,
 * received while the group leads, belongs here; a lower term is dropped, a
 * group that does not lead has no arm for it, and a higher term goes to
 * qe_vote_step as a QE_VMSG_VOTE_RESP of that term with QE_VMF_REJECT
 * (becomeFollower(m.Term, None), QE_VR_STEPPED_DOWN: the same transition for
 * every response type).  MsgSnapStatus is local (term 0, node.ReportSnapshot):
 * whatever carries a MsgSnap reports it (qe_carry with QE_CARRY_SNAP_STATUS for
 * the receivers in the batch, the host's transport for the others), or a peer
 * whose MsgSnap was lost stays in StateSnapshot. */
int qe_progress_step(const qe_progress *p, const qe_peer_msgs *m, uint64_t *stats,
                     void *stream);

/* ABI 5: MsgReadIndex on every group's leader whose request[g] is 1
 * (stepLeader, raft/raft.go:1078-1096, sendMsgReadIndexResponse :1827-1843),
 * result[g] (QE_RI_*):
 *   IsSingleton (one voter in Voters[0], Voters[1] empty; tracker.go:158-160)
 *     -> QE_RI_RESPOND at index = committed;
 *   no entry of the leader's term committed yet (committedEntryInCurrentTerm,
 *     :1731-1733: term_start <= committed <= last_index on the log model)
 *     -> QE_RI_POSTPONED (pendingReadIndexMessages; the host keeps the
 *     message and adds it again once qe_progress_step reports term_commit --
 *     its read index is that round's term_commit_index, NOT the index the
 *     re-added qe_read_index call returns: releasePendingReadIndexMessages
 *     runs inside the commit, before later advances of the same round);
 *   lease_based (ReadOnlyLeaseBased) -> QE_RI_RESPOND at committed;
 *   ReadOnlySafe -> readOnly.addRequest(committed) + the leader's own ack
 *     (self_slot; recvAck(r.id)): QE_RI_QUEUED with context number ctx[g]
 *     and index = committed; the host sends the heartbeats carrying ctx and
 *     answers when qe_progress_step releases the entry.  ABI 7: with keys
 *     (key and p->read_keys non-NULL) a request whose key[g] equals a
 *     pending request's is ignored, as addRequest ignores a context already
 *     pending (read_only.go:57-60; etcd's server resends the same request
 *     id, server/etcdserver/v3_server.go:808-824) -> QE_RI_DUPLICATE with
 *     that request's context.  With read_cap (QE_READ_QUEUE when 0)
 *     requests already pending (or the context numbers exhausted: read_head
 *     + read_count would be 0 mod 2^32) -> QE_RI_FULL, nothing changes (a
 *     capacity the host chose; up to QE_READ_CAP_MAX).
 * Needs p->read_acks / read_head / read_count unless every result is
 * RESPOND or POSTPONED (lease_based).  ctx and index may be NULL; they are
 * written only where they apply.  Groups without a request: result 0.
 * qe_read_note keeps the index and the origin of a QUEUED request on the
 * device, and qe_read_states lists the answers (below, after qe_ready). */
#define QE_RI_NONE 0
#define QE_RI_RESPOND 1
#define QE_RI_POSTPONED 2
#define QE_RI_QUEUED 3
#define QE_RI_FULL 4
#define QE_RI_DUPLICATE 5  /* ABI 7: key[g] is pending already: addRequest
                              ignores it (read_only.go:57-60); ctx[g] = the
                              pending request's context (the heartbeats the
                              reference sends then carry it), index not set */
int qe_read_index(const qe_progress *p, const uint8_t *request, const uint64_t *key,
                  uint32_t lease_based, uint8_t *result, uint32_t *ctx, uint64_t *index,
                  void *stream);

/* MsgCheckQuorum on every group's leader (stepLeader, raft/raft.go:997-1018):
 * the leader's own Progress (self_slot, when tracked) becomes RecentActive;
 * quorum_active[g] = ProgressTracker.QuorumActive() (raft/tracker/
 * tracker.go:215-225: Voters.VoteResult with each voter's vote = its
 * RecentActive, a voter without a Progress missing) -- 0 means the leader
 * steps down (becomeFollower); then RecentActive = false for every tracked
 * slot but the leader's (prs.Visit, raft.go:1013-1017).  Reads inc_mask /
 * out_mask / tracked / self_slot and the peer words of p.  A slot row in
 * which some group's word changes is rewritten for every tracked slot of
 * the tile, unchanged words included (whole sectors; the values written are
 * the round's result either way), so concurrent writers of other words of
 * p->peer must not overlap the call.  self_slot NULL (or >= S) means the
 * leader has no Progress of its own (the reference then marks nobody
 * active, raft.go:1000-1002): a caller whose leader has a slot must pass
 * it, or the leader is not counted as active.  quorum_active may be NULL.
 * stats: groups, stepdowns (QE_STAT_STEPDOWNS), checksum. */
int qe_check_quorum(const qe_progress *p, uint8_t *quorum_active, uint64_t *stats,
                    void *stream);

/* ABI 6: MsgBeat on every group's leader (stepLeader, raft/raft.go:991-993):
 * bcastHeartbeat (:524-541) -- one MsgHeartbeat to every tracked slot but
 * self_slot, each carrying Commit = min(Progress.Match, raftLog.committed)
 * (sendHeartbeat :494-510: a follower is never told a commit beyond what it
 * matched) and the context of the newest pending ReadIndex request
 * (lastPendingRequestCtx, read_only.go:114-121).  commit[s*stride + g]
 * (DEVICE, [S][stride]) is written for every slot sent to; ctx[g] (may be
 * NULL) = that context number, 0 when nothing is pending or p->read_acks is
 * NULL; sent[g] (mask-typed, may be NULL) = the slots sent to.  Reads
 * match, committed, tracked, self_slot and the ReadIndex queue's head and
 * count; writes nothing of p. */
int qe_heartbeat(const qe_progress *p, uint64_t *commit, uint32_t *ctx, void *sent, void *stream);

/* raft.tick() on every group (additive; the ABI version does not change):
 * tickElection (raft/raft.go:645-654) where state[g] != QE_STATE_LEADER,
 * tickHeartbeat (:657-684) where it leads -- the per-group gate in front of
 * MsgHup, MsgCheckQuorum and MsgBeat, with the latter two executed in the same
 * pass exactly as qe_check_quorum / qe_heartbeat execute them on that group.
 *
 * The timers: electionElapsed and heartbeatElapsed are 16-bit counters that
 * saturate at 65535.  A saturating 16-bit counter compares against any
 * threshold <= 65535 exactly as the reference's int does, and the largest
 * threshold is randomizedElectionTimeout <= 2*election_timeout - 1: hence
 * election_timeout <= 32768, the only bound.
 *
 * Per group, in this order:
 *  1. events[g] (what happened since the last tick): QE_TEV_HEARD ->
 *     electionElapsed = 0; QE_TEV_RESET -> both counters 0 and
 *     randomizedElectionTimeout drawn again (RESET wins over HEARD).  With
 *     ticks == 0 the call ends here for the group, action[g] = 0.
 *  2. state != leader (tickElection): electionElapsed++; if promotable()
 *     (:1618-1621) and pastElectionTimeout() (:1711-1713: electionElapsed >=
 *     randomizedElectionTimeout): electionElapsed = 0, QE_TICK_HUP.  The
 *     campaign (its pending-conf-change check, becomeCandidate's reset())
 *     stays with the caller -- qe_election_steps' script_hup or the host --
 *     which reports the reset() back as QE_TEV_RESET.  promotable: self_slot[g]
 *     < S, that slot in `tracked` (NULL = every slot) and in inc_mask |
 *     out_mask (NULL inc_mask = every slot a voter; LearnersNext sit in
 *     out_mask and count), and no_campaign[g] == 0; NULL self_slot = nobody.
 *  3. state == leader (tickHeartbeat): both counters++.  electionElapsed >=
 *     election_timeout -> electionElapsed = 0 and
 *       with QE_TICK_CHECK_QUORUM, MsgCheckQuorum (:997-1018, see
 *       qe_check_quorum): QE_TICK_CHECKED_QUORUM, quorum_active[g] written;
 *       not active -> becomeFollower(r.Term, None): state = follower, both
 *       counters 0, the timeout drawn again, lead_transferee = none,
 *       QE_TICK_STEPDOWN.  r.lead = None of that becomeFollower is the HOST's:
 *       qe_tick has no access to qe_follower.lead, so the host stores 0xFF
 *       there before the group's next qe_vote_step (a stale lead keeps the
 *       lease of raft.go:853-863 closed and canVote false).  The Votes masks
 *       need nothing: qe_vote_step clears them on the next campaign or term
 *       change.  The peer words are left as qe_check_quorum leaves
 *       them: the wholesale Progress reset of reset() (:600-616) is
 *       qe_become_leader's, the next time the group leads;
 *       still leader with lead_transferee[g] < S -> abortLeaderTransfer
 *       (:669-671).  QE_TICK_TRANSFER_ABORTED whenever the stored transferee
 *       went from a slot to none, by either path.
 *     No longer leader: nothing more (no beat on a stepdown tick).
 *     heartbeatElapsed >= heartbeat_timeout -> heartbeatElapsed = 0, MsgBeat:
 *     QE_TICK_BEAT and the outputs of qe_heartbeat for the group (hb_commit
 *     rows of the slots sent to, hb_ctx, hb_sent).
 *  4. a draw is election_timeout + ((hash4(seed, group_offset + g,
 *     (uint32_t)tick_no, 0x7131) >> 32) * election_timeout >> 32), hash4(seed,
 *     gid, lane, stream) = mix64(mix64(seed + gid * 0x9E3779B97F4A7C15) ^
 *     ((stream << 32 | lane) * 0xD6E8FEB86659FD93)), mix64 the splitmix64
 *     finalizer: uniform over [election_timeout, 2*election_timeout - 1] as
 *     the reference's globalRand.Intn (:1718-1720), a function of the global
 *     group id and the tick number alone (shards and replays agree).
 * Reads of p: inc_mask / out_mask / tracked / self_slot, peer (CheckQuorum),
 * match / committed and the ReadIndex queue's head and count (beats); writes
 * peer words and lead_transferee.  hb_sent[g] = 0 and nothing else of hb_* is
 * written where there is no beat; quorum_active only where the check ran.
 * stats: QE_STAT_GROUPS, QE_STAT_ELECTIONS (HUPs), QE_STAT_STEPDOWNS,
 * QE_STAT_CHECKSUM += mix64((group_offset + g) * 0x9E3779B97F4A7C15 ^
 * 0xA0761D6478BD642F ^ action << 56 ^ randomized_timeout << 32 ^ timer), the
 * values after the tick.
 * QE_EINVAL: a NULL p / t / out / state / timer / randomized_timeout /
 * action, a timeout out of range, unknown flag bits, ticks > 1, out_mask
 * without inc_mask, QE_TICK_CHECK_QUORUM with ticks == 1 and no p->peer,
 * hb_commit without p->match / p->committed or with stride < num_groups,
 * read_acks without read_head / read_count.  num_groups == 0 is QE_OK. */
#define QE_TICK_CHECK_QUORUM 1u      /* qe_timers.flags: raft.Config.CheckQuorum */

/* events[g], applied before the tick */
#define QE_TEV_HEARD 1u   /* electionElapsed = 0: a follower got MsgApp/MsgHeartbeat/
                             MsgSnap from its leader (raft.go:1434-1442), granted a
                             vote (:971), or the leader accepted MsgTransferLeader (:1362) */
#define QE_TEV_RESET 2u   /* the timer part of raft.reset() (:597-599): both elapsed
                             counters 0, randomizedElectionTimeout drawn again
                             (becomeFollower/Candidate/Leader) */

/* action[g] */
#define QE_TICK_HUP 1u              /* tickElection fired: the host steps MsgHup      */
#define QE_TICK_BEAT 2u             /* MsgBeat ran: hb_* outputs are valid for g      */
#define QE_TICK_CHECKED_QUORUM 4u   /* MsgCheckQuorum ran on g                        */
#define QE_TICK_STEPDOWN 8u         /* ... and QuorumActive was false                 */
#define QE_TICK_TRANSFER_ABORTED 16u/* lead_transferee went from a slot to none       */

typedef struct qe_timers {
  uint8_t  *state;              /* [G] rw QE_STATE_*; the tick writes it only on a stepdown */
  uint32_t *timer;              /* [G] rw: electionElapsed bits 0-15, heartbeatElapsed
                                   bits 16-31, each saturating at 65535 */
  uint16_t *randomized_timeout; /* [G] rw r.randomizedElectionTimeout */
  const uint8_t *no_campaign;   /* [G] or NULL: raftLog.hasPendingSnapshot() */
  const uint8_t *events;        /* [G] or NULL: QE_TEV_* */
  uint32_t election_timeout;    /* Config.ElectionTick, 1..32768 */
  uint32_t heartbeat_timeout;   /* Config.HeartbeatTick, 1..65535 */
  uint32_t flags;               /* QE_TICK_CHECK_QUORUM; other bits -> QE_EINVAL */
  uint32_t ticks;               /* 1 = one tick; 0 = apply events only */
  uint64_t seed;                /* of the timeout draw */
  uint64_t tick_no;             /* the host's tick counter, the draw's counter */
} qe_timers;

typedef struct qe_tick_out {
  uint8_t  *action;      /* [G] QE_TICK_* (required) */
  uint64_t *hb_commit;   /* [S][stride], as the commit of the MsgBeat entry point; NULL =
                            beats reported in action only */
  uint32_t *hb_ctx;      /* [G] or NULL */
  void     *hb_sent;     /* [G] mask-typed or NULL; 0 where no beat */
  uint8_t  *quorum_active; /* [G] or NULL; written only where CHECKED_QUORUM */
} qe_tick_out;

int qe_tick(const qe_progress *p, const qe_timers *t, const qe_tick_out *out,
            uint64_t *stats, void *stream);

/* The follower's half (additive; the ABI version does not change): one
 * MsgApp or MsgHeartbeat per group stepped through the term preamble of
 * raft.Step (raft/raft.go:847-920), stepFollower / stepCandidate's arms for
 * the two messages (:1390-1395, :1433-1440), handleAppendEntries and
 * handleHeartbeat (:1475-1516) and becomeFollower / reset (:590-619, :686-693)
 * on the group's log: the term runs of qe_progress, the same rows the group
 * uses when it leads.  MsgVote / MsgPreVote, their responses and MsgTimeoutNow
 * are qe_vote_step's (below); MsgSnap (restore rebuilds the configuration) is
 * qe_snapshot_step's (further below).
 *
 * Of p it reads num_groups, group_offset, stride, log_runs, num_slots (only to
 * validate `from`) and reads and WRITES committed, last_index, run_first,
 * run_term, run_count (declared const in qe_progress for the leader's entry
 * points; like qe_propose and qe_become_leader this one casts the const away)
 * and, when non-NULL, lead_transferee (0xFF where becomeFollower runs).  No
 * other field of p is touched: Progress rows, rings, masks and term_start stay
 * as they are (the Progress reset of reset() is qe_become_leader's, as for
 * qe_tick's stepdown).  The log: entries [run_first[0] + 1, last_index],
 * run_first[0] the dummy (snapshot) index, term(i) = run_term of the highest
 * run r < run_count with run_first[r] <= i, and 0 outside [run_first[0],
 * last_index] (raft/log.go:265-285).  The caller keeps raftLog's invariant
 * run_first[0] <= committed <= last_index < 2^64 - 1, run_first ascending,
 * run_count in 1..log_runs (results are unspecified otherwise; memory stays in
 * bounds).  2^64 - 1 is QE_INDEX_INF here as everywhere else in this ABI: the
 * reference cannot continue past it (Next = lastIndex + 1 and firstIndex =
 * snapshot index + 1 wrap), so no message may bring a log there (rule 2, and
 * qe_snapshot_step's).
 * Rows r >= run_count[g] are not state: the call may leave or overwrite them.
 *
 * Per group, in this order (m = the message, r = the group):
 *  1. type == QE_LMSG_NONE: result QE_FR_NONE, nothing else of the group is
 *     read or written (but events[g] = 0, see below).
 *  2. QE_FR_BAD_MSG (refused): an unknown type, from >= num_slots, and for a
 *     MsgApp a run with ent_len > 0 and ent_term 0, run terms that decrease
 *     (over the runs with ent_len > 0), or index + n wrapping or reaching
 *     2^64 - 1 (QE_INDEX_INF is no log index: see the invariant above).
 *  3. m.term < r.term (:883-919): with QE_FOLLOW_CHECK_QUORUM or
 *     QE_FOLLOW_PREVOTE QE_FR_LOWER_TERM_RESP (the empty MsgAppResp of :906),
 *     else QE_FR_IGNORED.  Nothing changes, no event.
 *  4. m.term > r.term (:876-877): becomeFollower(m.term, from): term = m.term,
 *     vote = none (0xFF), state = follower, lead = from, lead_transferee = none,
 *     event QE_TEV_RESET.
 *  5. m.term == r.term: a candidate or pre-candidate becomes follower as in 4
 *     but keeps its vote (reset() clears it only on a term change),
 *     QE_TEV_RESET; a leader -> QE_FR_IGNORED (stepLeader has no arm for
 *     these), nothing changes; a follower: lead = from, QE_TEV_HEARD.
 *  6. MsgHeartbeat: commitTo(m.commit) (never decreases committed); m.commit >
 *     last_index is the reference's panic (log.go:236-238) ->
 *     QE_FR_COMMIT_PAST_LOG (refused); else QE_FR_HEARTBEAT_RESP.
 *  7. MsgApp, entries index+1 .. index+n as term runs (run j: ent_len[j]
 *     entries of ent_term[j], n = the sum):
 *     index < committed -> QE_FR_APP_STALE, resp_index = committed (:1476-1479).
 *     term(index) != log_term -> QE_FR_APP_REJECT: resp_index = index,
 *       reject_hint = findConflictByTerm(min(index, last_index), log_term)
 *       (log.go:147-168), resp_log_term = term(reject_hint).
 *     else lastnewi = index + n and ci = findConflict (log.go:127-138): the
 *       first entry index whose term differs from the log's (an index past
 *       last_index differs), 0 when the log holds every entry.
 *       ci > last_index + 1 (possible only for index > last_index with
 *       log_term 0, which term() "matches") would leave a hole: the
 *       reference's slice-bounds panic in truncateAndAppend -> QE_FR_APP_GAP
 *       (refused).  ci != 0 && ci <= committed: the panic of log.go:94-95 ->
 *       QE_FR_CONFLICT_COMMITTED (refused).
 *       ci != 0: last_index = lastnewi; runs with run_first >= ci are dropped
 *       (kept rows are not rewritten); the pieces of the message's runs from
 *       ci on are appended in order, a zero-length piece skipped, a piece
 *       whose term equals the table's last run's term extending that run, any
 *       other piece a new run starting at its first index; more than log_runs
 *       rows -> QE_FR_RUNS_FULL (refused: qe_compact drops the runs below the
 *       applied index on the device and the host re-delivers, as for
 *       QE_BL_RUNS_FULL).  ci == 0: the log is not truncated, even
 *       when it is longer than lastnewi.
 *       commitTo(min(m.commit, lastnewi)); past last_index (only the index >
 *       last_index, log_term 0, n = 0 message) -> QE_FR_COMMIT_PAST_LOG.
 *       QE_FR_APP_ACCEPT, resp_index = lastnewi, append_from = ci.
 *  8. A refused group (result >= 16): nothing but result is written -- the
 *     effects of 4 / 5 and the event are dropped too.
 * Outputs: result[g] for every group.  events[g] (when non-NULL) for every
 * group too, 0 where no event was raised (NONE, lower term, ignored, refused),
 * so the array is a complete qe_timers.events for the next qe_tick.  For a
 * group with 0 < result < 16: resp_index (0 for IGNORED / LOWER_TERM_RESP /
 * HEARTBEAT_RESP) and append_from (ci of an accept, else 0); reject_hint and
 * resp_log_term only where result == QE_FR_APP_REJECT.  The heartbeat's
 * context is not an input: the response echoes it, the host copies it.
 * Building the MsgAppResp / MsgHeartbeatResp of a result from these rows is
 * optional for a host now: qe_replies lists these messages on the device.
 * stats (over the groups with type != NONE): QE_STAT_GROUPS += 1;
 * QE_STAT_GRANTED += result == APP_ACCEPT; QE_STAT_REJECTED += result ==
 * APP_REJECT; QE_STAT_FOLLOW_APPENDED += lastnewi - ci + 1 where ci != 0;
 * QE_STAT_COMMIT_ADVANCED += committed rose; QE_STAT_INVARIANT_VIOLATIONS +=
 * result >= 16; QE_STAT_CHECKSUM += h4, h1 = mix64((group_offset + g) *
 * 0x9E3779B97F4A7C15 ^ 0x2545F4914F6CDD1D ^ result << 56), h2 = mix64(h1 ^
 * term), h3 = mix64(h2 ^ committed), h4 = mix64(h3 ^ last_index), the values
 * after the call.
 * QE_EINVAL: a NULL p / f / m / out / result / term / state / lead / type /
 * from / m.term / index / log_term / commit / committed / last_index /
 * run_first / run_term / run_count, msg_runs > QE_MAX_MSG_RUNS, msg_runs > 0
 * without ent_len / ent_term, log_runs 0 or > QE_MAX_LOG_RUNS, stride <
 * num_groups, unknown flag bits.  num_groups == 0 is QE_OK. */
#define QE_MAX_MSG_RUNS 4
#define QE_FOLLOW_CHECK_QUORUM 1u   /* qe_follower.flags: raft.Config.CheckQuorum */
#define QE_FOLLOW_PREVOTE 2u        /* raft.Config.PreVote */
#define QE_LMSG_NONE 0
#define QE_LMSG_APP 1
#define QE_LMSG_HEARTBEAT 2
#define QE_FR_NONE 0
#define QE_FR_IGNORED 1             /* no response */
#define QE_FR_LOWER_TERM_RESP 2     /* MsgAppResp{} (:906) */
#define QE_FR_HEARTBEAT_RESP 3      /* MsgHeartbeatResp */
#define QE_FR_APP_ACCEPT 4          /* MsgAppResp{Index: resp_index} */
#define QE_FR_APP_REJECT 5          /* MsgAppResp{Index, Reject, RejectHint, LogTerm} */
#define QE_FR_APP_STALE 6           /* MsgAppResp{Index: committed} */
#define QE_FR_REFUSED 16            /* results >= this: nothing of the group changed */
#define QE_FR_BAD_MSG 16
#define QE_FR_COMMIT_PAST_LOG 17
#define QE_FR_CONFLICT_COMMITTED 18
#define QE_FR_RUNS_FULL 19
#define QE_FR_APP_GAP 20
#define QE_STAT_FOLLOW_APPENDED QE_STAT_COMMIT_SUM /* qe_follower_step: entries appended */

typedef struct qe_follower {
  uint64_t *term;        /* [G] rw r.Term */
  uint8_t  *state;       /* [G] rw QE_STATE_*, the row qe_timers.state uses */
  uint8_t  *lead;        /* [G] rw slot of r.lead, >= num_slots = None */
  uint8_t  *vote;        /* [G] rw or NULL: slot of r.Vote, >= num_slots = None */
  uint32_t flags;        /* QE_FOLLOW_*; other bits -> QE_EINVAL */
  uint32_t reserved;
} qe_follower;

typedef struct qe_leader_msgs {
  const uint8_t  *type;      /* [G] QE_LMSG_* */
  const uint8_t  *from;      /* [G] the sender's slot */
  const uint64_t *term;      /* [G] m.Term */
  const uint64_t *index;     /* [G] m.Index */
  const uint64_t *log_term;  /* [G] m.LogTerm */
  const uint64_t *commit;    /* [G] m.Commit */
  uint32_t msg_runs;         /* E, 0..QE_MAX_MSG_RUNS */
  uint32_t reserved;
  const uint32_t *ent_len;   /* [E][stride] entries of run j */
  const uint64_t *ent_term;  /* [E][stride] their term */
} qe_leader_msgs;

typedef struct qe_follower_out {
  uint8_t  *result;        /* [G] QE_FR_* (required) */
  uint64_t *resp_index;    /* [G] or NULL */
  uint64_t *reject_hint;   /* [G] or NULL */
  uint64_t *resp_log_term; /* [G] or NULL */
  uint64_t *append_from;   /* [G] or NULL */
  uint8_t  *events;        /* [G] or NULL: QE_TEV_* */
} qe_follower_out;

int qe_follower_step(const qe_progress *p, const qe_follower *f, const qe_leader_msgs *m,
                     const qe_follower_out *out, uint64_t *stats, void *stream);

/* ---- elections: votes, campaigns, tallies (additive in ABI 8) ------------- */
/* The election between two leaderships on the resident state: one MsgVote /
 * MsgPreVote / MsgVoteResp / MsgPreVoteResp / MsgHup / MsgTimeoutNow per group
 * stepped through the term preamble of raft.Step with its lease check
 * (raft/raft.go:849-920), the vote decision (:930-978), stepCandidate's
 * response arm (:1399-1414, RecordVote / TallyVotes), hup / campaign (:760-835)
 * and the header part of becomeFollower / becomePreCandidate / becomeCandidate
 * / becomeLeader.  The chain: qe_tick raises QE_TICK_HUP -> qe_vote_step (HUP)
 * campaigns -> the host sends the requests -> qe_vote_step on the voters ->
 * the host sends the responses -> qe_vote_step on the candidate (WON) ->
 * qe_become_leader(out->elected, f->term) -> qe_follower_step on the others.
 * One message per group per call; a host with several messages for one group
 * makes several calls, in its delivery order.
 *
 * f is qe_follower_step's struct; vote is required here, f->flags is not read.
 * Of p the call reads num_groups, group_offset, stride, num_slots, log_runs,
 * last_index, run_first, run_term, run_count, inc_mask, out_mask, tracked,
 * self_slot and writes lead_transferee only (when non-NULL).  The log, the
 * Progress rows and the rings are never written.  lastTerm = term(last_index)
 * by the definition above; with the invariant run_first[run_count - 1] <=
 * last_index, which every reachable log has, it is run_term[run_count - 1],
 * the only run row the kernel reads.  A slot byte (lead, vote, self_slot)
 * >= num_slots is None.
 *
 * The lease compares electionElapsed (bits 0-15 of the qe_timers.timer row)
 * with election_timeout: pending events must have been applied first (qe_tick
 * with ticks == 0).  The saturating 16-bit counter compares exactly because
 * election_timeout <= 32768.
 *
 * Per group, in this order (m = the message, r = the group, S = num_slots):
 *  1. type == QE_VMSG_NONE: QE_VR_NONE, nothing of the group is read or
 *     written (events[g] = elected[g] = 0).
 *  2. QE_VR_BAD_MSG (refused): an unknown type; from >= S or m.term == 0 for
 *     every type but HUP; a response, HUP or TIMEOUT_NOW when voted, granted or
 *     p->self_slot is NULL (a voter-only launch); HUP / TIMEOUT_NOW with
 *     self_slot[g] >= S.
 *  3. The term preamble (not for HUP, whose term is not read).
 *     m.term > r.term: inLease = QE_VOTE_CHECK_QUORUM && lead < S &&
 *       electionElapsed < election_timeout; a request in lease without
 *       QE_VMF_FORCE -> QE_VR_IN_LEASE, nothing changes.  A PREVOTE, and a
 *       PREVOTE_RESP without QE_VMF_REJECT, never change the term (:865-872).
 *       Everything else (VOTE, VOTE_RESP, a rejecting PREVOTE_RESP,
 *       TIMEOUT_NOW): becomeFollower(m.term, None) -- term = m.term, vote =
 *       none (0xFF), state = follower, lead = none, lead_transferee = none,
 *       voted = granted = 0 (when non-NULL), event QE_TEV_RESET ("3d").
 *     m.term < r.term: a PREVOTE -> QE_VR_REJECT with resp_term = r.term
 *       (:907-913); anything else -> QE_VR_IGNORED.  Nothing changes.
 *  4. Requests, in any state (:930-978): canVote = vote == from || (vote ==
 *     none && lead == none) || (PREVOTE && m.term > r.term); up to date =
 *     log_term > lastTerm || (log_term == lastTerm && index >= last_index).
 *     Both -> QE_VR_GRANT, resp_term = m.term; for a VOTE only vote = from and
 *     QE_TEV_HEARD (electionElapsed = 0, :971) unless RESET was raised.  Else
 *     QE_VR_REJECT, resp_term = r.term (after 3d).  Learners vote: there is no
 *     membership check.
 *  5. Responses (:1399-1414): nothing is done unless the type is the state's
 *     own (VOTE_RESP <-> candidate, PREVOTE_RESP <-> pre-candidate).  RecordVote:
 *     the first vote of `from` sticks, its value !QE_VMF_REJECT.  TallyVotes =
 *     JointConfig.VoteResult over inc_mask / out_mask (NULL inc_mask = every
 *     slot); a voter outside the masks is recorded, not counted.  Pending ->
 *     QE_VR_PENDING.  Lost -> becomeFollower(r.term, None): the vote is kept,
 *     state = follower, lead = lead_transferee = none, voted = granted = 0,
 *     RESET, QE_VR_LOST.  Won as candidate -> 7; won as pre-candidate -> the
 *     campaign of 6 as campaignElection.
 *  6. HUP (hup, :760-781) does nothing on a leader, on a group that is not
 *     promotable (qe_tick's rule: self_slot < S, in tracked, in inc | out) or
 *     with no_campaign[g] set.  TIMEOUT_NOW: only a follower (after the
 *     preamble) goes on, as hup(campaignTransfer); a transfer never pre-votes.
 *     The campaign (:785-835): HUP under QE_VOTE_PREVOTE -> becomePreCandidate
 *     (state = pre-candidate, lead = none, voted = granted = the self bit; term,
 *     vote, lead_transferee and the timers untouched, no event); the tally won
 *     (a single voter) -> on as an election, else QE_VR_CAMPAIGN_PREVOTE with
 *     resp_term = r.term + 1.  An election or a transfer -> becomeCandidate
 *     (term + 1, vote = self, lead = lead_transferee = none, state = candidate,
 *     voted = granted = the self bit, RESET); the tally won -> 7, else
 *     QE_VR_CAMPAIGN_VOTE with resp_term = the new term.  Both campaign results
 *     write req_log_term = lastTerm and req_to = (inc | out) & ~self: the host
 *     sends Msg{Pre}Vote{Term: resp_term, Index: last_index, LogTerm:
 *     req_log_term} to req_to and adds the transfer context to a campaign it
 *     began with TIMEOUT_NOW.  Both are optional now: qe_replies lists the
 *     requests, with QE_VMF_FORCE where the campaign began with TIMEOUT_NOW.
 *  7. Won (becomeLeader's header part): state = leader, lead = self,
 *     lead_transferee = none, voted = granted = 0, RESET, elected[g] = 1,
 *     QE_VR_WON.  The Progress reset, the empty entry and the bcast are
 *     qe_become_leader's: the host calls it next with out->elected and f->term.
 *  8. The arm did nothing: QE_VR_STEPPED_DOWN when 3d ran, else QE_VR_IGNORED.
 *  9. A refused group (result >= 16): nothing but result is written.
 * Outputs: result, and when non-NULL elected and events, for every group
 * (elected 1 only where result == WON; events 0 where none was raised): they
 * are a complete qe_leader.elected and qe_timers.events row.  resp_term only
 * for GRANT / REJECT / CAMPAIGN_*; req_log_term and req_to only for CAMPAIGN_*.
 * Sending the Msg{Pre}VoteResp of a GRANT / REJECT and the requests of a
 * campaign from these rows is optional for a host now: qe_replies lists these
 * messages on the device.
 * stats (over the groups with type != NONE): QE_STAT_GROUPS += 1;
 * QE_STAT_GRANTED += result == GRANT; QE_STAT_REJECTED += result == REJECT;
 * QE_STAT_VOTE_PENDING += result == PENDING; QE_STAT_ELECTIONS +=
 * becomeCandidate or becomePreCandidate ran from a hup or TIMEOUT_NOW;
 * QE_STAT_LEADERS += result == WON; QE_STAT_STEPDOWNS += result == LOST, and
 * += 3d ran; QE_STAT_INVARIANT_VIOLATIONS += result >= 16; QE_STAT_CHECKSUM
 * += h4, h1 = mix64((group_offset + g) * 0x9E3779B97F4A7C15 ^
 * 0x9FB21C651E98DF25 ^ result << 56), h2 = mix64(h1 ^ term), h3 = mix64(h2 ^
 * (state | lead << 8 | vote << 16 | events << 24)), h4 = mix64(h3 ^ (voted |
 * granted << 16)), the values after the call, the masks 0 when NULL.
 * QE_EINVAL: a NULL p / f / v / m / out / result / term / state / lead / vote
 * / type / from / m.term / index / log_term / last_index / run_term /
 * run_first / run_count, QE_VOTE_CHECK_QUORUM without timer, election_timeout
 * outside 1..32768, unknown flag bits, out_mask without inc_mask, exactly one
 * of voted / granted NULL, log_runs 0 or > QE_MAX_LOG_RUNS, stride <
 * num_groups.  num_groups == 0 is QE_OK. */
#define QE_VMSG_NONE 0
#define QE_VMSG_VOTE 1            /* MsgVote */
#define QE_VMSG_PREVOTE 2         /* MsgPreVote */
#define QE_VMSG_VOTE_RESP 3       /* MsgVoteResp */
#define QE_VMSG_PREVOTE_RESP 4    /* MsgPreVoteResp */
#define QE_VMSG_HUP 5             /* local MsgHup; the message term is not read */
#define QE_VMSG_TIMEOUT_NOW 6     /* MsgTimeoutNow */
#define QE_VMF_FORCE 1u           /* a request: Context == campaignTransfer */
#define QE_VMF_REJECT 2u          /* a response: m.Reject */
#define QE_VOTE_CHECK_QUORUM 1u   /* qe_voter.flags: raft.Config.CheckQuorum */
#define QE_VOTE_PREVOTE 2u        /* raft.Config.PreVote */
#define QE_VR_NONE 0
#define QE_VR_IGNORED 1           /* no response */
#define QE_VR_IN_LEASE 2          /* a request dropped by the lease */
#define QE_VR_GRANT 3             /* Msg{Pre}VoteResp{Term: resp_term} */
#define QE_VR_REJECT 4            /* Msg{Pre}VoteResp{Term: resp_term, Reject} */
#define QE_VR_STEPPED_DOWN 5      /* becomeFollower(m.term, None) and nothing else */
#define QE_VR_PENDING 6           /* the vote is recorded, the tally is open */
#define QE_VR_LOST 7
#define QE_VR_CAMPAIGN_PREVOTE 8  /* send MsgPreVote to req_to */
#define QE_VR_CAMPAIGN_VOTE 9     /* send MsgVote to req_to */
#define QE_VR_WON 10              /* call qe_become_leader next */
#define QE_VR_REFUSED 16          /* results >= this: nothing of the group changed */
#define QE_VR_BAD_MSG 16

typedef struct qe_voter {
  const uint32_t *timer;      /* [G] the qe_timers.timer row, read only
                                 (electionElapsed = bits 0-15); required with
                                 QE_VOTE_CHECK_QUORUM */
  uint32_t election_timeout;  /* 1..32768 */
  uint32_t flags;             /* QE_VOTE_*; other bits -> QE_EINVAL */
  void *voted, *granted;      /* [G] rw mask-typed or both NULL: the Votes map
                                 (the rows qe_election_state uses); NULL = a
                                 voter-only launch */
  const uint8_t *no_campaign; /* [G] or NULL: non-zero = hup() returns early (a
                                 pending snapshot or unapplied conf changes,
                                 raft.go:770-777) */
} qe_voter;

typedef struct qe_vote_msgs {
  const uint8_t  *type;      /* [G] QE_VMSG_* */
  const uint8_t  *from;      /* [G] the sender's slot */
  const uint64_t *term;      /* [G] m.Term */
  const uint64_t *index;     /* [G] m.Index (requests) */
  const uint64_t *log_term;  /* [G] m.LogTerm (requests) */
  const uint8_t  *flags;     /* [G] QE_VMF_*, or NULL = all 0 */
} qe_vote_msgs;

typedef struct qe_vote_out {
  uint8_t  *result;        /* [G] QE_VR_* (required) */
  uint64_t *resp_term;     /* [G] or NULL */
  uint64_t *req_log_term;  /* [G] or NULL */
  void     *req_to;        /* [G] mask-typed or NULL */
  uint8_t  *elected;       /* [G] or NULL: a complete qe_leader.elected row */
  uint8_t  *events;        /* [G] or NULL: a complete qe_timers.events row */
} qe_vote_out;

int qe_vote_step(const qe_progress *p, const qe_follower *f, const qe_voter *v,
                 const qe_vote_msgs *m, const qe_vote_out *out, uint64_t *stats, void *stream);

/* raft.sendAppend / maybeSendAppend(to, send_if_empty) once for the slots of
 * want[g] (raft.go:432-492; bcastAppend after a proposal is want = every
 * tracked slot but the leader's, send_if_empty = 1): paused peers get
 * nothing; with no entries to send (Next > lastIndex, or Next < firstIndex
 * where entries() fails with ErrCompacted) nothing is sent unless
 * send_if_empty -- this check comes before the snapshot branch; Next >
 * lastIndex sends an empty MsgApp; Next < firstIndex sends a MsgSnap to a
 * recently active peer (BecomeSnapshot(snap_index)); otherwise up to
 * p->max_ents entries (0 = noLimit; ABI 3 takes MaxSizePerMsg from p, as
 * qe_progress_step does): Replicate -> OptimisticUpdate + Inflights.Add,
 * Probe -> ProbeSent.  sent / snap (mask-typed [G], may be NULL) report the
 * outcome. */
int qe_progress_send(const qe_progress *p, const void *want, uint32_t send_if_empty,
                     void *sent, void *snap, void *stream);

/* ---- MsgProp: appendEntry + bcastAppend (ABI 6) ------------------------- */

/* qe_proposals.result */
#define QE_PROP_NONE 0                /* no proposal for the group             */
#define QE_PROP_OK 1                  /* appended and bcastAppend done          */
#define QE_PROP_DROPPED_NOT_MEMBER 2  /* ErrProposalDropped: the leader has no
                                         Progress of its own (raft.go:1023-1028) */
#define QE_PROP_DROPPED_TRANSFER 3    /* ErrProposalDropped: leadership transfer
                                         in progress (raft.go:1029-1032)       */
#define QE_PROP_DROPPED_SIZE 4        /* ErrProposalDropped: the uncommitted
                                         size limit (raft.go:627-633, 1761-1779) */
#define QE_PROP_BAD_CC 5              /* ABI 7: cc_count[g] > max_cc -- refused
                                         whole, nothing changes (an input error
                                         reported per group, never clamped)    */
#define QE_PROP_MAX_CC 8              /* conf-change entries per proposal      */
/* qe_proposals.flags: appendEntry alone, as the reference calls it outside
 * MsgProp (the auto-leave entry of advance, raft.go:555-569; tests'
 * mustAppendEntry): no MsgProp gates except the leader's own Progress, no
 * conf-change checks (max_cc ignored), no bcastAppend */
#define QE_PROP_APPEND_ONLY 1u

/* One MsgProp per group (a launch is one batch of proposals). */
typedef struct qe_proposals {
  const uint32_t *num_entries;   /* [G] len(m.Entries); 0 = no MsgProp         */
  const uint64_t *payload;       /* [G] sum of PayloadSize (len(Data), util.go)
                                    over the entries that are NOT conf
                                    changes; NULL = all of them empty       */
  uint32_t max_cc;               /* conf-change entries per proposal at most,
                                    <= QE_PROP_MAX_CC (0: no conf changes)  */
  uint32_t flags;                /* QE_PROP_APPEND_ONLY or 0                  */
  uint64_t cc_stride;            /* >= num_groups                            */
  const uint8_t *cc_count;       /* [G] conf-change entries of the proposal
                                    (> max_cc: QE_PROP_BAD_CC)              */
  const uint32_t *cc_pos;        /* [max_cc][cc_stride] position in m.Entries,
                                    ascending, < num_entries                */
  const uint8_t *cc_leave;       /* [max_cc][cc_stride] 1: a ConfChangeV2
                                    without Changes (wantsLeaveJoint)        */
  const uint32_t *cc_size;       /* [max_cc][cc_stride] its PayloadSize      */
  const uint64_t *applied;       /* [G] raftLog.applied (read when a group has
                                    conf-change entries)                    */
  uint64_t *pending_conf_index;  /* [G] rw r.pendingConfIndex (ditto)        */
  uint64_t *uncommitted_size;    /* [G] rw r.uncommittedSize; NULL = not
                                    tracked (max_uncommitted must be 0)     */
  uint64_t max_uncommitted;      /* Config.MaxUncommittedEntriesSize; 0 =
                                    noLimit (raft.go:356-358)               */
  uint8_t *result;               /* [G] out QE_PROP_*                         */
  uint8_t *cc_refused;           /* [G] out (may be NULL): bit k = conf-change
                                    entry k was refused and replaced by an
                                    empty EntryNormal (raft.go:1063-1065)   */
  void *sent;                    /* [G] out mask (may be NULL): peers sent a
                                    MsgApp / MsgSnap by the bcastAppend     */
  void *snap;                    /* [G] out mask (may be NULL): a MsgSnap     */
  uint64_t *bytes_requested;     /* measurement aid, normally NULL: adds the
                                    algorithmic bytes (DESIGN.md §3 rules)  */
} qe_proposals;

/* stepLeader's MsgProp arm (raft/raft.go:1019-1076) for every group with
 * num_entries > 0, on the leader-side state p (p->self_slot is required:
 * MsgProp needs the leader's own id, QE_EINVAL without it):
 *   the leader has no Progress of its own (self_slot untracked) -> dropped;
 *   a leadership transfer is in progress (lead_transferee < S) -> dropped;
 *   each conf-change entry in order: refused (replaced by an empty
 *     EntryNormal) when pendingConfIndex > applied, or it enters a change
 *     while Voters[1] is non-empty, or it leaves a joint state that does not
 *     exist; otherwise pendingConfIndex = its index (set even when the
 *     proposal is then dropped for its size, as the reference does);
 *   appendEntry (:621-642): increaseUncommittedSize -> dropped when the
 *     uncommitted tail is non-empty, the proposal's payload is non-zero and
 *     the sum would exceed max_uncommitted; else lastIndex += num_entries
 *     (the entries take the leader's term: the log model's current run,
 *     [term_start, last_index], grows), Progress[self].MaybeUpdate(lastIndex)
 *     and maybeCommit (the term gate of qe_progress_step);
 *   bcastAppend (:515-522): sendAppend (maybeSendAppend(to, true)) to every
 *     tracked slot but self_slot, as qe_progress_send.
 * Writes p->last_index (declared const in qe_progress because the other
 * entry points only read it), p->committed, the leader's Match/Next/word and
 * the peers' Next/word/PendingSnapshot/Inflights.  The reference's
 * reduceUncommittedSize on apply (:544) stays with the host, which owns the
 * applied entries.  stats: groups, commit sum, commit advanced, checksum. */
int qe_propose(const qe_progress *p, const qe_proposals *prop, uint64_t *stats, void *stream);

/* ---- becomeLeader (ABI 7) ----------------------------------------------- */

/* qe_leader.result */
#define QE_BL_NONE 0        /* elected[g] == 0: not part of this call           */
#define QE_BL_LEADER 1      /* becomeLeader done                                */
#define QE_BL_NOT_MEMBER 2  /* self_slot holds no Progress: the reference would
                               panic (a candidate is promotable, so a voter);
                               nothing changes                               */
#define QE_BL_RUNS_FULL 3   /* a run of the new term would have to be appended
                               and run_count == log_runs: nothing changes
                               (qe_compact frees rows on the device, then
                               retry).  A full table whose last run already
                               has term[g] (a bootstrap snapshot of the new
                               leader's own term) appends nothing and is no
                               refusal: QE_BL_LEADER                         */
#define QE_BL_BCAST 1u      /* qe_leader.flags: then bcastAppend, as
                               stepCandidate does after winning (raft.go:
                               1405-1407)                                     */

typedef struct qe_leader {
  const uint8_t *elected;        /* [G] 1: the group's node won its election
                                    (NULL = every group)                      */
  const uint64_t *term;          /* [G] r.Term of the new leadership           */
  uint32_t flags;                /* QE_BL_BCAST or 0                           */
  uint32_t reserved;             /* must be 0                                  */
  uint64_t *pending_conf_index;  /* [G] out (may be NULL): r.pendingConfIndex =
                                    lastIndex before the empty entry         */
  uint64_t *uncommitted_size;    /* [G] out (may be NULL): 0 (reset; the empty
                                    entry is not counted, raft.go:753-757)   */
  uint8_t *result;               /* [G] out QE_BL_*                            */
  void *sent;                    /* [G] out mask (may be NULL): bcastAppend's  */
  void *snap;                    /* [G] out mask (may be NULL)                 */
} qe_leader;

/* raft.becomeLeader (raft/raft.go:724-759) on every group with elected[g],
 * on the leader-side state p:
 *   reset (:590-613): every tracked slot's Progress becomes Match 0, Next =
 *     lastIndex + 1, StateProbe, not ProbeSent, not RecentActive, no pending
 *     snapshot, empty Inflights; the leader's own (self_slot) Match =
 *     lastIndex, then BecomeReplicate; lead_transferee = none; the ReadIndex
 *     queue emptied (newReadOnly: read_count 0, read_head past the dropped
 *     requests' context numbers, so a late response for one finds nothing);
 *   pendingConfIndex = lastIndex; uncommittedSize = 0;
 *   the log model enters the term: a run [lastIndex + 1, ...) of term[g] is
 *     appended to the run table and term_start = lastIndex + 1 -- unless the
 *     last run has term[g] already: run_count stays and term_start = that
 *     run's first index;
 *   appendEntry of the empty entry (:621-642): lastIndex + 1, the leader's
 *     MaybeUpdate, maybeCommit (a one-voter config commits it at once);
 *   QE_BL_BCAST: bcastAppend (every tracked slot but the leader's, the
 *     probes of a new term).
 * Writes p's Progress rows, Inflights words, committed, last_index,
 * term_start, the run table (run_first / run_term / run_count) and
 * lead_transferee / the queue when present (declared const in qe_progress
 * because the other entry points only read them).  stats: groups, commit
 * sum, commit advanced, checksum. */
int qe_become_leader(const qe_progress *p, const qe_leader *l, uint64_t *stats, void *stream);

/* ---- switchToConfig: the leader's side of an applied conf change (ABI 7) - */

/* qe_switch.result & QE_SW_OUTCOME */
#define QE_SW_NONE 0       /* switched[g] == 0: not part of this call           */
#define QE_SW_REMOVED 1    /* the leader has no Progress any more, or is a
                              learner: switchToConfig returns at once
                              (raft.go:1663-1674; the leader stays leader)    */
#define QE_SW_NO_VOTERS 2  /* Voters[0] is empty: returns (:1678-1680)         */
#define QE_SW_BCAST 3      /* maybeCommit advanced the commit under the new
                              config: bcastAppend (:1682-1685)                  */
#define QE_SW_PROBE 4      /* it did not: maybeSendAppend(id, false) to every
                              tracked peer (:1686-1692)                         */
#define QE_SW_OUTCOME 0x0Fu
#define QE_SW_TRANSFER_ABORTED 0x10u /* result bit: leadTransferee was not a voter
                                        of the new config, abortLeaderTransfer
                                        (:1694-1697)                            */

typedef struct qe_switch {
  const uint8_t *switched;       /* [G] 1: the group's configuration was just
                                    switched (its conf change applied); NULL =
                                    every group                               */
  uint8_t *result;               /* [G] out QE_SW_* (| QE_SW_TRANSFER_ABORTED) */
  void *sent;                    /* [G] out mask (may be NULL): peers sent a
                                    MsgApp / MsgSnap                          */
  void *snap;                    /* [G] out mask (may be NULL): a MsgSnap      */
  uint64_t *bytes_requested;     /* measurement aid, normally NULL: adds the
                                    algorithmic bytes (DESIGN.md §3 rules)    */
} qe_switch;

/* raft.switchToConfig (raft/raft.go:1651-1700) after the new configuration
 * is in place -- inc_mask / out_mask / tracked of p are the new Voters[0],
 * Voters[1] and ProgressMap keys (e.g. the qe_conf masks qe_confchange just
 * wrote) -- for every group with switched[g]:
 *   the leader (self_slot) has no Progress, or is a learner (tracked but in
 *     neither half: Learners, confchange.go checkInvariants) -> QE_SW_REMOVED;
 *   Voters[0] empty -> QE_SW_NO_VOTERS;
 *   maybeCommit under the new JointConfig (the term gate of qe_progress_step)
 *     advanced -> bcastAppend: sendAppend (sendIfEmpty) to every tracked slot
 *     but the leader's; else maybeSendAppend(id, false) to every tracked slot
 *     (prs.Visit: the leader's own included -- a no-op while its Next is
 *     lastIndex + 1, as appendEntry keeps it);
 *   then a lead_transferee that is not in Voters[0] | Voters[1] is cleared
 *     (abortLeaderTransfer) and QE_SW_TRANSFER_ABORTED set.
 * As in the reference, this maybeCommit does not release postponed ReadIndex
 * requests (only stepLeader's MsgAppResp arm calls
 * releasePendingReadIndexMessages, :1259-1262).  Writes committed, the
 * peers' Next / word / PendingSnapshot / Inflights and lead_transferee.
 * stats: groups, commit sum, commit advanced, checksum. */
int qe_switch_config(const qe_progress *p, const qe_switch *sw, uint64_t *stats, void *stream);

/* ABI 4, HOST pointers: Inflights rings between plain uint64 buffers
 * (Inflights.buffer of each peer, raft/tracker/inflights.go:25-37, peer-major
 * [S][stride][F]: entry k of slot s of group g at (s*stride + g)*F + k) and
 * the device form (infl_lo / infl_hi, pitch QE_RING_PITCH(F)).  qe_ring_pack
 * also writes each peer word's ring representation bits (QE_PW_RING_MASK,
 * canonical form; the other bits are kept: Inflights.start / count must be
 * set).  qe_ring_unpack decodes all F entries of every peer (positions
 * outside the live window decode like live ones; their values are whatever
 * the ring holds there, as in the reference).  Groups [0, num_groups). */
int qe_ring_pack(uint64_t num_groups, uint32_t num_slots, uint32_t inflight_cap,
                 uint64_t stride, const uint64_t *entries, uint32_t *peer,
                 uint32_t *infl_lo, uint32_t *infl_hi);
int qe_ring_unpack(uint64_t num_groups, uint32_t num_slots, uint32_t inflight_cap,
                   uint64_t stride, const uint32_t *infl_lo, const uint32_t *infl_hi,
                   const uint32_t *peer, uint64_t *entries);
/* ABI 8, HOST pointers: the same for the 16-bit form (qe_progress.infl16):
 * Next ([S][stride], next) is the base of each peer's offsets.  Every peer
 * gets the 16-bit form when its live entries fit below its Next, else the
 * wide form (infl_lo / infl_hi, QE_PF_RING_WIDE); infl_lo / infl_hi are
 * written for every peer.  inflight_cap <= QE_RING16_MAX_F. */
int qe_ring_pack16(uint64_t num_groups, uint32_t num_slots, uint32_t inflight_cap,
                   uint64_t stride, const uint64_t *entries, const uint64_t *next,
                   uint32_t *peer, uint16_t *infl16, uint32_t *infl_lo, uint32_t *infl_hi);
int qe_ring_unpack16(uint64_t num_groups, uint32_t num_slots, uint32_t inflight_cap,
                     uint64_t stride, const uint16_t *infl16, const uint32_t *infl_lo,
                     const uint32_t *infl_hi, const uint64_t *next, const uint32_t *peer,
                     uint64_t *entries);

/* ---- sparse MsgAppResp deltas ------------------------------------------ */

/* Apply n MsgAppResp acks in COO form -- ack i: group[i], slot[i] (-1 =
 * skip), index[i] -- with Progress.MaybeUpdate semantics
 * (raft/tracker/progress.go:144-153): match = max(match, index),
 * next = max(next, index + 1), via 64-bit atomic max.  Max is commutative,
 * so duplicated or reordered acks give the same state as applying them one
 * by one in any order.  touched[g] (optional) is set to 1 for every group
 * that received an ack.  All pointers are device pointers. */
int qe_apply_append_resps(uint64_t num_groups, uint32_t num_slots, uint64_t stride,
                          uint64_t *match, uint64_t *next, uint64_t n, const uint64_t *group,
                          const int8_t *slot, const uint64_t *index, uint8_t *touched,
                          void *stream);

/* ---- host-side ConfState packing (wire format -> slot SoA) -------------- */

/* G ConfStates (raft/raftpb/raft.proto:115-130) in CSR form: list k of
 * group g is ids_k[off_k[g] .. off_k[g+1]).  NULL lists are empty.  HOST
 * pointers.  Produced by ProgressTracker.ConfState (tracker.go:146-154). */
typedef struct qe_confstate_csr {
  uint64_t num_groups;
  const uint64_t *voters, *voters_off;
  const uint64_t *voters_outgoing, *outgoing_off;
  const uint64_t *learners, *learners_off;
  const uint64_t *learners_next, *learners_next_off;
  const uint8_t *auto_leave;    /* [G] ConfState.auto_leave (ABI 2; NULL = false) */
  const uint64_t *perm;         /* ABI 3: packed position i takes the caller's
                                   group perm[i] (qe_pack_order); NULL =
                                   identity.  Every packer output is in
                                   packed order. */
} qe_confstate_csr;

/* group_flags bits reported by qe_pack_confstate */
#define QE_PACK_TOO_MANY_PEERS 1u          /* > num_slots peers: group left empty */
#define QE_PACK_LEARNER_IS_VOTER 2u        /* confchange.go:308-318 violated      */
#define QE_PACK_LEARNER_NEXT_NOT_OUTGOING 4u /* confchange.go:299-306 violated   */
#define QE_PACK_ZERO_ID 8u                 /* ID 0 is raft.None                   */

/* Shape bucketing (ABI 3; the order the JointConfig kernels want, DESIGN.md
 * §2): perm[i] = the caller's group placed at packed position i, groups
 * sorted by configuration shape -- (|Voters[0] u Voters[1]|, |Voters[0]|,
 * |Voters[1]|, learners) ascending, caller order within a shape (stable);
 * groups the packer would flag sort last.  With cs->perm = perm the groups
 * of one shape fill consecutive 64-group tiles: every lane of a wave has its
 * voters in the same low slots (voters are placed first), so the joint
 * commit kernel fetches exactly the union's slot rows.  Quorum results are
 * order-free per group; the host maps packed outputs back through perm
 * (qe_collect does it on the device).  *num_shapes (optional) = distinct
 * shapes.  perm is a HOST array of num_groups entries. */
int qe_pack_order(const qe_confstate_csr *cs, uint32_t num_slots, uint64_t *perm,
                  uint64_t *num_shapes);

/* Slot assignment: voters of both halves ascending, then learners ascending.
 * Writes the three masks (mask-typed, may be NULL), slot_ids (ABI 3:
 * ID-major [S][G], slot s of packed group i at slot_ids[s*G + i]; 0 =
 * unused slot) and optional per-group flags; *num_flagged counts flagged
 * groups.  Outputs are in packed order (cs->perm).  Multi-threaded
 * (qe_pack_threads). */
int qe_pack_confstate(const qe_confstate_csr *cs, uint32_t num_slots, void *inc_mask,
                      void *out_mask, void *learner_mask, uint64_t *slot_ids,
                      uint32_t *group_flags, uint64_t *num_flagged);

/* Progress.Match of each peer (CSR prog_ids/prog_match, in the caller's
 * group order) into match[S][stride] (host, packed order); packed group i
 * reads CSR row perm[i] (NULL = identity; ABI 3).  slot_ids as written by
 * qe_pack_confstate ([S][G]).  Peers without a slot are counted in
 * *num_unknown. */
int qe_pack_match(uint64_t num_groups, uint32_t num_slots, const uint64_t *slot_ids,
                  const uint64_t *perm, const uint64_t *prog_off, const uint64_t *prog_ids,
                  const uint64_t *prog_match, uint64_t *match, uint64_t stride,
                  uint64_t *num_unknown);

/* ProgressTracker.Votes (CSR vote_ids / vote_vals 0|1, caller order) into
 * voted/granted bitmaps (packed order, through perm as qe_pack_match); the
 * first vote per peer sticks (tracker.go:258-263). */
int qe_pack_votes(uint64_t num_groups, uint32_t num_slots, const uint64_t *slot_ids,
                  const uint64_t *perm, const uint64_t *vote_off, const uint64_t *vote_ids,
                  const uint8_t *vote_vals, void *voted, void *granted);

/* (packed group, id) -> slot (-1 if the id has no slot) for routing deltas;
 * slot_ids [S][G].  A caller that bucketed maps its group id to the packed
 * position with the inverse of perm. */
int qe_slot_lookup(uint64_t num_groups, uint32_t num_slots, const uint64_t *slot_ids,
                   uint64_t n, const uint64_t *group, const uint64_t *id, int8_t *slot);

/* Host packing threads (0 = min(16, hardware threads)). */
int qe_pack_threads(int n);

/* ---- configuration changes (raft/confchange/confchange.go) ------------- */

/* ConfChangeSingle.Type (raft/raftpb/raft.pb.go:224-227) */
#define QE_CC_ADD_NODE 0
#define QE_CC_REMOVE_NODE 1
#define QE_CC_UPDATE_NODE 2
#define QE_CC_ADD_LEARNER_NODE 3

/* per-group operation */
#define QE_CC_OP_NONE 0
#define QE_CC_OP_SIMPLE 1            /* Changer.Simple          (:130-147) */
#define QE_CC_OP_ENTER_JOINT 2       /* Changer.EnterJoint(false, ...)     */
#define QE_CC_OP_ENTER_JOINT_AUTO 3  /* Changer.EnterJoint(true, ...) (:49-76) */
#define QE_CC_OP_LEAVE_JOINT 4       /* Changer.LeaveJoint      (:92-123) */

/* per-group result (a group with an error keeps its state, as the caller of
 * the reference Changer discards the returned config on error) */
#define QE_CC_OK 0
#define QE_CC_ERR_INVARIANT 1        /* checkInvariants on the input (:186-241) */
#define QE_CC_ERR_ALREADY_JOINT 2    /* "config is already joint"              */
#define QE_CC_ERR_ZERO_VOTER_JOINT 3 /* "can't make a zero-voter config joint" */
#define QE_CC_ERR_NOT_JOINT 4        /* "can't leave a non-joint config"       */
#define QE_CC_ERR_SIMPLE_IN_JOINT 5  /* "can't apply simple config change in joint config" */
#define QE_CC_ERR_BAD_TYPE 6         /* "unexpected conf type %d"              */
#define QE_CC_ERR_REMOVED_ALL 7      /* "removed all voters"                   */
#define QE_CC_ERR_SIMPLE_MULTI 8     /* "more than one voter changed without entering joint config" */
#define QE_CC_ERR_INVARIANT_OUT 9    /* checkInvariants on the result          */
#define QE_CC_ERR_NO_SLOT 10         /* slot model: a new peer found no free slot */

/* tracker.Config + the ProgressMap key set of G groups in slot form.  A slot
 * is tracked when it holds a Progress (ProgressMap key); Voters[0],
 * Voters[1], Learners and LearnersNext are slot masks ([G], u8 for
 * num_slots <= 8, else u16) over tracked slots; is_learner is
 * Progress.IsLearner.  slot_ids is ID-major [S][G] (ABI 3: slot s of group
 * g at slot_ids[s*G + g]) as written by qe_pack_confstate, so a change
 * rewrites only the changed slot's row.  The ids of untracked slots are
 * ignored on input (qe_confchange) and left as they are, except that a slot
 * a change untracks gets 0; the packer writes 0 for every unused slot.
 * qe_pack_match / qe_pack_votes / qe_slot_lookup match ids over all S slots,
 * so a caller that writes slot_ids itself keeps untracked ones 0. */
typedef struct qe_conf {
  uint64_t num_groups;
  uint32_t num_slots;
  uint32_t reserved;
  uint64_t *slot_ids;           /* [S][G]                                   */
  void *inc_mask, *out_mask;    /* Voters[0], Voters[1]                     */
  void *learner_mask;           /* Learners                                 */
  void *learners_next_mask;     /* LearnersNext                             */
  void *is_learner;             /* Progress.IsLearner                       */
  void *tracked;                /* slots holding a Progress                 */
  uint8_t *auto_leave;          /* [G] Config.AutoLeave                     */
} qe_conf;

/* The whole tracker.Config of each group from its ConfState, as
 * ProgressTracker.ConfState / confchange.Restore see it (raft/tracker/
 * tracker.go:146-154, raft/confchange/restore.go:1-155): slot_ids (voters of
 * both halves ascending, then learners), Voters[0], Voters[1], Learners,
 * LearnersNext (outgoing voters only), Progress.IsLearner (= Learners; a
 * LearnersNext peer is still a voter), tracked (every placed peer) and
 * AutoLeave -- the state qe_confchange consumes.  All pointers in `out` are
 * HOST pointers here (copy them to the device for qe_confchange); its
 * num_groups must equal cs->num_groups.  Flagged groups (QE_PACK_*) are left
 * empty. */
int qe_pack_conf(const qe_confstate_csr *cs, const qe_conf *out, uint32_t *group_flags,
                 uint64_t *num_flagged);

/* One operation per group with up to max_changes ConfChangeSingle entries:
 * change c of group g at [c*stride + g]. */
typedef struct qe_conf_changes {
  uint32_t max_changes;
  uint32_t reserved;
  uint64_t stride;              /* >= num_groups                            */
  const uint8_t *op;            /* [G] QE_CC_OP_*                           */
  const uint8_t *count;         /* [G] changes of group g (<= max_changes)  */
  const uint8_t *type;          /* [C][stride] QE_CC_ADD_NODE ...           */
  const uint64_t *node_id;      /* [C][stride] NodeID (0 = ignored, :154-160) */
  const uint64_t *last_index;   /* [G] Changer.LastIndex                    */
  uint8_t *result;              /* [G] out: QE_CC_*                         */
  void *new_progress;           /* [G] out mask (may be NULL): slots whose
                                   Progress initProgress created           */
} qe_conf_changes;

/* Changer.Simple / EnterJoint / LeaveJoint per group (raft/confchange/
 * confchange.go:49-274): makeVoter, makeLearner (LearnersNext while the
 * peer is an outgoing voter), remove (keeps the Progress of an outgoing
 * voter), symdiff over voter ids, checkInvariants before and after.  A new
 * peer takes the lowest untracked slot.  When `p` is non-NULL (same G and S)
 * the Progress of every created slot is initialised as initProgress does
 * (:262-273): Match 0, Next = last_index, StateProbe, RecentActive, empty
 * Inflights, no pending snapshot. */
int qe_confchange(const qe_conf *c, const qe_conf_changes *ch, const qe_progress *p,
                  void *stream);

/* ---- snapshots: the log's lower end (additive in ABI 8) ------------------- */
/* qe_compact: MemoryStorage.CreateSnapshot and MemoryStorage.Compact
 * (raft/storage.go:194-236) on the term-run log of p, per group create then
 * compact, as etcd's server does it.  Of p it reads num_groups, group_offset,
 * stride, log_runs, committed, last_index and reads and WRITES run_first,
 * run_term, run_count and, when non-NULL, first_index and snap_index (declared
 * const in qe_progress; cast away as qe_follower_step does).  committed,
 * last_index, term_start, the Progress rows and the rings are never touched: a
 * leader's next send sees Next < firstIndex by itself.
 *   bound = min(applied[g], committed[g]), committed[g] with no applied row.
 *     The reference leaves "not past applied" to the application
 *     (storage.go:215-217); the engine enforces it, which also keeps
 *     run_first[0] <= committed.
 *   Create, i = create_index[g] != 0 (storage.go:194-213):
 *     i <= snap_index[g] -> bit QE_CP_SNAP_OUT_OF_DATE (ErrSnapOutOfDate :197-199),
 *       nothing changes for this operation;
 *     else i > last_index (the panic of :202-204) or i < run_first[0] (the
 *       slice index of :207 below zero) -> QE_CP_OUT_OF_BOUND (refused);
 *     else i > bound -> QE_CP_PAST_APPLIED (refused);
 *     else snap_index[g] = i, snap_term[g] = term(i) (:206-207), bit
 *       QE_CP_CREATED.
 *   Compact, ci = compact_index[g] != 0 (storage.go:218-236):
 *     ci <= run_first[0] -> bit QE_CP_ALREADY (ErrCompacted :222-224), nothing
 *       changes;
 *     ci > last_index (the panic of :225-227) -> QE_CP_OUT_OF_BOUND (refused);
 *     ci > bound -> QE_CP_PAST_APPLIED (refused);
 *     else with r* the highest run below run_count with run_first[r*] <= ci
 *       (:229-234): row 0 becomes (ci, run_term[r*]), row k >= 1 becomes the old
 *       row r* + k, run_count -= r*, first_index[g] = ci + 1, bit
 *       QE_CP_COMPACTED.  With r* == 0 only run_first[0] is stored: a kept row
 *       is never rewritten (the contract of qe_follower_step).  Rows >= the new
 *       run_count are not state and keep their bytes.
 *   A result >= QE_CP_REFUSED: nothing of the group changed, the effects of the
 *   other operation included; where both operations refuse, the create's code
 *   stands.  The bits below 16 combine.
 * result[g] is written for every group (QE_CP_NONE without a request).
 * stats (over the groups with a request): QE_STAT_GROUPS += 1;
 * QE_STAT_COMPACTED += ci - the old run_first[0] where compacted;
 * QE_STAT_INVARIANT_VIOLATIONS += result >= 16; QE_STAT_CHECKSUM += h4, h1 =
 * mix64((group_offset + g) * 0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03 ^ result
 * << 56), h2 = mix64(h1 ^ run_first[0]), h3 = mix64(h2 ^ run_count), h4 =
 * mix64(h3 ^ snap_index) (0 without the row), the values after the call.
 * QE_EINVAL: a NULL p / c / compact_index / result / committed / last_index /
 * run_first / run_term / run_count, create_index given with p->snap_index NULL,
 * log_runs 0 or > QE_MAX_LOG_RUNS, stride < num_groups.  num_groups == 0 is
 * QE_OK. */
#define QE_CP_NONE 0
#define QE_CP_CREATED 1u            /* snap_index / snap_term written */
#define QE_CP_COMPACTED 2u          /* the dummy row moved to compact_index */
#define QE_CP_SNAP_OUT_OF_DATE 4u   /* ErrSnapOutOfDate */
#define QE_CP_ALREADY 8u            /* ErrCompacted */
#define QE_CP_REFUSED 16            /* results >= this: nothing of the group changed */
#define QE_CP_OUT_OF_BOUND 16
#define QE_CP_PAST_APPLIED 17
#define QE_STAT_COMPACTED QE_STAT_COMMIT_SUM /* qe_compact: entries compacted */

typedef struct qe_compaction {
  const uint64_t *compact_index; /* [G] Compact(ci); 0 = none                */
  const uint64_t *create_index;  /* [G] or NULL; CreateSnapshot(i); 0 = none */
  const uint64_t *applied;       /* [G] or NULL                              */
  uint64_t *snap_term;           /* [G] out or NULL: term(i) where created   */
  uint8_t  *result;              /* [G] out, required                        */
} qe_compaction;

int qe_compact(const qe_progress *p, const qe_compaction *c, uint64_t *stats, void *stream);

/* qe_snapshot_step: one MsgSnap per group stepped through the term preamble of
 * raft.Step (raft/raft.go:849-920), the MsgSnap arms of stepFollower /
 * stepCandidate (:1396-1398, :1441-1444) and handleSnapshot / restore
 * (:1518-1614) with raftLog.restore (raft/log.go:333-337) and
 * confchange.Restore (raft/confchange/restore.go:21-155).
 *
 * p is the receiver's log as in qe_follower_step, plus first_index and
 * snap_index (written when non-NULL) and self_slot (required).  c is the
 * group's tracker.Config in slot form with DEVICE pointers; its inc_mask,
 * out_mask and tracked rows are normally the very buffers p points at (the
 * rows qe_vote_step and qe_tick read).  The ConfState of the message comes in
 * the RECEIVER's slot numbering: slot assignment stays with the host, and a
 * peer present before and after the restore keeps its slot.  The engine cannot
 * check this.
 *
 * Per group, in this order (m = the message, r = the group):
 *  1. type == QE_SMSG_NONE: QE_SR_NONE, nothing else of the group is read or
 *     written (but events[g] = 0).
 *  2. QE_SR_BAD_MSG (refused): an unknown type, from >= num_slots, or
 *     snap_index == 2^64 - 1 (QE_INDEX_INF is no log index: first_index =
 *     snap_index + 1 would wrap).
 *  3. The preamble, as steps 3-5 of qe_follower_step, except that m.term <
 *     r.term is ALWAYS QE_SR_IGNORED, whatever CheckQuorum and PreVote say:
 *     :884 lists only MsgApp and MsgHeartbeat (so qe_follower's flags are not
 *     read).  m.term > r.term: becomeFollower(m.term, from), QE_TEV_RESET.
 *     Equal terms: a candidate or pre-candidate becomes follower and keeps its
 *     vote (:1396-1398), QE_TEV_RESET; a leader -> QE_SR_IGNORED (stepLeader
 *     has no MsgSnap arm), nothing changes; a follower: lead = from,
 *     QE_TEV_HEARD (:1441-1444).
 *  4. sindex <= committed (:1535-1537) -> QE_SR_STALE, resp_index = committed.
 *  5. The self bit is not in cs_inc | cs_learner | cs_out, or self_slot >=
 *     num_slots (:1554-1580) -> QE_SR_NOT_MEMBER, resp_index = committed.
 *  6. term(sindex) == sterm by the run table (matchTerm, :1584-1589):
 *     commitTo(sindex), QE_SR_FAST_FORWARD, resp_index = sindex.  term() is 0
 *     outside the log, so sterm == 0 with sindex > last_index "matches" and
 *     would commit past the log (the panic of log.go:236-238) ->
 *     QE_SR_COMMIT_PAST_LOG (refused), as QE_FR_APP_GAP's case.
 *  7. A ConfState confchange.Restore fails on, or whose result is not
 *     equivalent to it (assertConfStatesEquivalent), is the reference's panic
 *     (:1600-1606) -> QE_SR_BAD_CONF (refused).  In mask form: cs_inc == 0
 *     with cs_out | cs_learner != 0 (the all-empty ConfState restores to the
 *     empty configuration without error, but step 5 answers it first);
 *     (cs_inc | cs_out) & cs_learner != 0; cs_learners_next not a subset of
 *     cs_out & ~cs_inc; cs_out == 0 with cs_learners_next != 0 or
 *     cs_auto_leave set; a bit at or past num_slots in any of the four.
 *  8. Restore -> QE_SR_RESTORED, resp_index = sindex: committed = last_index =
 *     sindex; the run table is the single row (sindex, sterm), run_count 1;
 *     first_index = sindex + 1 and snap_index = sindex where those rows are
 *     non-NULL; every non-NULL row of c is written for the group: the four
 *     masks, is_learner = cs_learner, tracked = cs_inc | cs_out | cs_learner,
 *     auto_leave (0 / 1) and, with cs_ids and slot_ids, the id of each tracked
 *     slot and 0 for an untracked one.  The Progress rows and the rings are
 *     not written (as in qe_follower_step: reset() in qe_become_leader
 *     rewrites them before anything reads them).  The host sets no_campaign[g]
 *     until it has applied the snapshot (hasPendingSnapshot in promotable, :1618-1621).
 *  9. A refused group (result >= 16): nothing but result is written -- the
 *     effects of 3 and the event are dropped too.
 * Outputs: result[g] and events[g] (when non-NULL) for every group, events 0
 * where none was raised, so the array is a complete qe_timers.events row.
 * resp_index only where a MsgAppResp goes out: STALE, NOT_MEMBER,
 * FAST_FORWARD, RESTORED.  Sending that MsgAppResp from the rows is optional
 * for a host now: qe_replies lists these messages on the device.
 * stats (over the groups with type != NONE): QE_STAT_GROUPS += 1;
 * QE_STAT_GRANTED += RESTORED; QE_STAT_REJECTED += STALE or NOT_MEMBER;
 * QE_STAT_COMMIT_ADVANCED += committed rose; QE_STAT_INVARIANT_VIOLATIONS +=
 * result >= 16; QE_STAT_CHECKSUM += h4 of qe_follower_step's chain (result,
 * term, committed, last_index after the call) with the constant
 * 0x8CB92BA72F3D8DD7.
 * QE_EINVAL: a NULL p / f / c / m / out / result / term / state / lead / type /
 * from / m.term / snap_index / snap_term / cs_inc / cs_out / cs_learner /
 * cs_learners_next / cs_auto_leave / committed / last_index / run_first /
 * run_term / run_count / self_slot, c->num_groups or c->num_slots other than
 * p's, c->reserved, stride < num_groups, log_runs 0 or > QE_MAX_LOG_RUNS.
 * num_groups == 0 is QE_OK. */
#define QE_SMSG_NONE 0
#define QE_SMSG_SNAP 1
#define QE_SR_NONE 0
#define QE_SR_IGNORED 1             /* no response */
#define QE_SR_STALE 2               /* MsgAppResp{Index: committed} */
#define QE_SR_NOT_MEMBER 3          /* MsgAppResp{Index: committed} */
#define QE_SR_FAST_FORWARD 4        /* MsgAppResp{Index: committed} after commitTo */
#define QE_SR_RESTORED 5            /* MsgAppResp{Index: lastIndex} */
#define QE_SR_REFUSED 16            /* results >= this: nothing of the group changed */
#define QE_SR_BAD_MSG 16
#define QE_SR_COMMIT_PAST_LOG 17
#define QE_SR_BAD_CONF 18

typedef struct qe_snap_msgs {
  const uint8_t  *type;        /* [G] 0 = none, 1 = MsgSnap */
  const uint8_t  *from;        /* [G] sender's slot */
  const uint64_t *term;        /* [G] m.Term */
  const uint64_t *snap_index, *snap_term;              /* [G] Metadata.Index / Term */
  const void *cs_inc, *cs_out, *cs_learner, *cs_learners_next; /* [G] mask-typed ConfState,
                                  in the RECEIVER's slot numbering */
  const uint8_t  *cs_auto_leave;  /* [G] */
  const uint64_t *cs_ids;         /* [S][stride] or NULL: peer id per slot */
} qe_snap_msgs;
typedef struct qe_snap_out { uint8_t *result; uint64_t *resp_index; uint8_t *events; } qe_snap_out;
int qe_snapshot_step(const qe_progress *p, const qe_follower *f, const qe_conf *c,
                     const qe_snap_msgs *m, const qe_snap_out *out, uint64_t *stats, void *stream);

/* ---- Ready deltas ------------------------------------------------------ */

/* The groups a batch step changed, as a dense list in ascending position
 * order: for every g with flags[g] != 0, out_groups[i] = group_offset + g
 * (ABI 3: group_offset + perm[g] when perm is non-NULL -- the caller's group
 * id of a shape-bucketed batch, qe_pack_order) and (when out_values is
 * non-NULL) out_values[i] = values[g]; *out_count (device) =
 * their number.  raft reports a HardState only when it changed
 * (raft/node.go:571-573 newReady, raft/rawnode.go:152-176 prevHardSt): with
 * flags = qe_replication_round's `adv` and values = `committed` this is the
 * per-round commit delta a host ships instead of all G words.  out_groups /
 * out_values hold up to num_groups entries (NULL: not written).  scratch:
 * qe_collect_scratch_bytes(num_groups) bytes of device memory, 8-B aligned.
 * All pointers are device pointers; stream-ordered. */
size_t qe_collect_scratch_bytes(uint64_t num_groups);
int qe_collect(uint64_t num_groups, uint64_t group_offset, const uint64_t *perm,
               const uint8_t *flags, const uint64_t *values, uint64_t *out_groups,
               uint64_t *out_values, uint64_t *out_count, void *scratch, void *stream);

/* qe_outbox (additive in ABI 8): the messages one leader-side call sent, as a
 * dense, ordered list of records on the device -- the Ready.Messages half of
 * the Ready whose commit half qe_collect lists.  The step entry points report
 * a send as mask bits (`sent`, `snap`, `hb_sent`) and a few rows (msg_index,
 * hb_commit, hb_ctx); this call turns the masks of ONE call into
 * MsgApp{Index, LogTerm, Entries, Commit} (maybeSendAppend, raft/raft.go:
 * 432-492: Index = pr.Next - 1, LogTerm = term(Index), the entries after it,
 * Commit = raftLog.committed; the MsgSnap arm with the snapshot's Metadata)
 * and MsgHeartbeat{Commit, Context} (sendHeartbeat / bcastHeartbeatWithCtx,
 * :495-532) records.  It READS the resident state of p and never writes it;
 * of p it reads num_groups, group_offset, num_slots, stride, log_runs,
 * committed, last_index, run_first, run_term, run_count and, by need, next,
 * peer, snap_index and first_index.
 *
 *  1. Mask.  Per group mask = (sent | snap | hb_sent) & ((1 << num_slots) - 1),
 *     a NULL mask array taken as 0.  Every set bit s yields exactly one record,
 *     of type QE_OMSG_SNAP where the snap bit is set, else QE_OMSG_APP where
 *     the sent bit is set, else QE_OMSG_HEARTBEAT.  The masks are those of one
 *     call (qe_progress_step's sent / snap, qe_tick's hb_sent, ...).
 *  2. Order.  Records are listed by ascending tile (g / 64), then slot, then g.
 *     The order is part of the contract; *count depends on the masks alone.
 *  3. Truncation.  A record at a position >= capacity is not written; *count
 *     is still the full number, and nothing at or past min(*count, capacity)
 *     is touched in any output array.
 *  4. QE_OMSG_APP.  index = in->index[s*stride+g] when `index` is given (the
 *     msg_index row of qe_progress_step).  Otherwise, for the entry points
 *     that report no index (qe_propose, qe_become_leader, qe_progress_send,
 *     qe_switch_config): next_before[s*stride+g] - 1 for a peer whose peer
 *     word says QE_PR_REPLICATE after the call (an optimistic send moved Next
 *     past the message, :468-477), p->next[s*stride+g] - 1 for every other
 *     state (a probe leaves Next alone); next_before is a copy of p->next
 *     taken before the call (p->next itself after qe_become_leader, where
 *     every peer probes).  With r0 = run_first[0]: an index outside
 *     [r0, last_index] (or a group with run_count 0) gives type QE_OMSG_BAD
 *     with `index` as computed and log_term, commit, ctx and the entry runs 0.
 *     Otherwise log_term = term(index) on the run table (raftLog.term),
 *     commit = committed[g], and the entries are (index, hi] with hi =
 *     min(last_index, index + (max_entries ? max_entries : 0xFFFFFFFF)), split
 *     into the term runs of the table: run j of the message is the j-th table
 *     run that overlaps (index, hi], ent_len[j*capacity+i] its overlap and
 *     ent_term[j*capacity+i] its term.  The message is cut after msg_runs
 *     runs: it then ends where its last listed run ends (with msg_runs 0 no
 *     entries are listed).  Unused ent_len / ent_term rows of a record are 0.
 *  5. QE_OMSG_SNAP.  index = snap_index[g] (first_index[g] - 1 when
 *     p->snap_index is NULL), log_term = in->snap_term[g], or term(index) on
 *     the run table (0 outside the log) when in->snap_term is NULL; commit 0,
 *     no runs.  The ConfState is not in the record: it belongs to the
 *     snapshot the application stored (Storage.Snapshot()), as for
 *     qe_snapshot_step's inputs.
 *  6. QE_OMSG_HEARTBEAT.  commit = hb_commit[s*stride+g], ctx = hb_ctx[g] (0
 *     with hb_ctx NULL); index and log_term 0, no runs.
 *  7. Every record, QE_OMSG_BAD included: group = group_offset + g, to = s,
 *     term = in->term[g] (the sender's r.Term); ctx is 0 for every type but
 *     the heartbeat.
 *  8. stats (optional), over every record the masks ask for, those past
 *     capacity too: QE_STAT_GROUPS += groups with a non-empty mask;
 *     QE_STAT_OUTBOX_APP / _SNAP / _HEARTBEAT / _BAD += records by type, BAD
 *     also into QE_STAT_INVARIANT_VIOLATIONS; QE_STAT_OUTBOX_ENTRIES += entries
 *     listed (the sum of a record's ent_len); QE_STAT_CHECKSUM += h5 per
 *     record, h1 = mix64((group_offset + g) * 0x9E3779B97F4A7C15 ^
 *     0xC2B2AE3D27D4EB4F ^ type << 56 ^ to << 48), h2 = mix64(h1 ^ index), h3 =
 *     mix64(h2 ^ log_term), h4 = mix64(h3 ^ commit), h5 = mix64(h4 ^ entries
 *     listed).
 * `count` and every array of qe_outbox_out are DEVICE pointers; scratch is
 * qe_outbox_scratch_bytes(num_groups) bytes of device memory, 8-B aligned.
 * Stream-ordered: three kernels (count per 4096-group chunk, the scan of
 * qe_collect, fill), no host synchronisation.
 * QE_EINVAL: a NULL p / in / out / scratch (with num_groups > 0) / count /
 * term; a NULL committed, last_index, run_first, run_term or run_count;
 * log_runs 0 or > QE_MAX_LOG_RUNS; stride < num_groups; `sent` given with
 * neither `index` nor `next_before`; next_before used (index NULL) with a NULL
 * p->next or p->peer; `snap` given with p->snap_index and p->first_index both
 * NULL; hb_sent without hb_commit; msg_runs > QE_MAX_MSG_RUNS, or > 0 without
 * ent_len / ent_term; capacity > 0 with a NULL group / to / type / term /
 * index / log_term / commit array (ctx may be NULL: not written); a nonzero
 * reserved field; scratch not 8-B aligned.  Every argument check runs before
 * the first HIP call.  num_groups == 0 is QE_OK with *count = 0.
 *
 * With this call duty H7 of a host (tests/cluster_sim.py: pick m.Index, look
 * up LogTerm, cut the entries into term runs, attach Commit and Term) is
 * optional: the host copies min(*count, capacity) records instead of the
 * G-sized and S x stride-sized rows it would walk. */
#define QE_OMSG_APP 1        /* MsgApp       */
#define QE_OMSG_SNAP 2       /* MsgSnap: index / log_term = Metadata.Index / Term */
#define QE_OMSG_HEARTBEAT 3  /* MsgHeartbeat */
#define QE_OMSG_BAD 255      /* a mask bit whose m.Index is outside the log */
#define QE_STAT_OUTBOX_ENTRIES QE_STAT_COMMIT_SUM    /* qe_outbox: entries listed */
#define QE_STAT_OUTBOX_APP QE_STAT_VOTE_WON          /* ... records by type */
#define QE_STAT_OUTBOX_SNAP QE_STAT_VOTE_LOST
#define QE_STAT_OUTBOX_HEARTBEAT QE_STAT_VOTE_PENDING
#define QE_STAT_OUTBOX_BAD QE_STAT_REJECTED

typedef struct qe_outbox_in {
  const void *sent, *snap, *hb_sent;   /* [G] mask-typed, each may be NULL */
  const uint64_t *index;        /* [S][stride] m.Index (qe_peer_msgs.msg_index), or NULL */
  const uint64_t *next_before;  /* [S][stride] Next as it was before the call, or NULL */
  const uint64_t *term;         /* [G] the sender's r.Term (qe_follower.term), required */
  const uint64_t *snap_term;    /* [G] or NULL: NULL = term(snap_index) from the runs */
  const uint64_t *hb_commit;    /* [S][stride], required with hb_sent */
  const uint32_t *hb_ctx;       /* [G] or NULL (ctx 0) */
  uint32_t max_entries;         /* entries per MsgApp at most, 0 = no limit */
  uint32_t reserved;            /* must be 0 */
} qe_outbox_in;

typedef struct qe_outbox_out {
  uint64_t capacity;            /* records the arrays hold */
  uint32_t msg_runs;            /* E, 0..QE_MAX_MSG_RUNS */
  uint32_t reserved;
  uint64_t *group;              /* [capacity] group_offset + g */
  uint8_t  *to, *type;          /* [capacity] slot, QE_OMSG_* */
  uint64_t *term, *index, *log_term, *commit;  /* [capacity] */
  uint32_t *ctx;                /* [capacity] or NULL */
  uint32_t *ent_len;            /* [E][capacity] */
  uint64_t *ent_term;           /* [E][capacity] */
  uint64_t *count;              /* device: records the masks ask for (may exceed capacity) */
} qe_outbox_out;

size_t qe_outbox_scratch_bytes(uint64_t num_groups);
int qe_outbox(const qe_progress *p, const qe_outbox_in *in, const qe_outbox_out *out,
              void *scratch, uint64_t *stats, void *stream);

/* qe_inbox (additive in ABI 8): a list of delivered messages routed into the
 * message rows of the step entry points -- the receive half of the loop whose
 * send half qe_outbox lists.  Every step entry point takes whole-batch rows
 * with at most one message per group (qe_progress_step: one per slot and
 * group); this call picks, per group, which records of the list go into this
 * pass of calls and which wait, runs raft.Step's term preamble for the
 * response types (qe_peer_msgs carries no term), turns a higher-term response
 * into the QE_VMSG_VOTE_RESP qe_progress_step's comment asks for, and scatters
 * the fields into the four row families.  It READS the list, f->term and
 * f->state; of p it reads num_groups (G), group_offset, num_slots (S) and
 * stride and nothing else.  It writes nothing resident: only the rows of
 * qe_inbox_out, which the caller points at the buffers it then passes to
 * qe_follower_step, qe_snapshot_step, qe_progress_step and qe_vote_step.
 *
 * The list is in delivery order; a record's position i is its rank.  Mapping
 * (sender group, `to` slot) to (receiver group, `from` slot) is the host's
 * table (qe_peers), as slot assignment stays with the host; qe_carry applies it
 * on the device for the receivers that share the batch.
 *
 *  1. Class.  QE_IMSG_APP and _HEARTBEAT are class F (qe_follower_step),
 *     QE_IMSG_SNAP is class S (qe_snapshot_step), QE_IMSG_APP_RESP ..
 *     _TRANSFER_LEADER are class R (qe_progress_step), QE_IMSG_VOTE .. _HUP are
 *     class V (qe_vote_step).  APP, SNAP and HEARTBEAT equal QE_OMSG_*: an
 *     outbox `type` array can be fed in unchanged.
 *  2. BAD.  A record whose group is outside [group_offset, group_offset + G),
 *     whose type is none of QE_IMSG_*, or whose from >= num_slots (any type
 *     but QE_IMSG_HUP) gets QE_ID_BAD.  It takes no further part and is not
 *     deferred.
 *  3. Wave forming.  Per group, over its remaining records in list order: the
 *     first record opens the group's wave and fixes the wave's class.  A later
 *     record joins the wave only if the group is still open, both it and the
 *     opener are class R, and no record already in the wave has the same
 *     `from`.  Otherwise the group closes: that record and every later record
 *     of the group get QE_ID_DEFERRED.
 *  4. HUP from the tick.  Where tick_action[g] & QE_TICK_HUP, the group's wave
 *     is opened by a virtual QE_IMSG_HUP record that stands before position 0:
 *     v_type[g] = QE_VMSG_HUP with from, term, index, log_term and flags 0 and
 *     v_src[g] = QE_INBOX_SRC_TICK, and every list record of g is deferred.
 *  5. Classes F, S, V.  The wave's one member is QE_ID_ROUTED as it is into
 *     its family's rows at [g]: f_type = QE_LMSG_APP / _HEARTBEAT with from,
 *     term, index, log_term, commit and, for an APP only, all msg_runs rows of
 *     f_ent_len / f_ent_term at [j*stride+g] (zeros included); s_type =
 *     QE_SMSG_SNAP with from, term, snap_index = index, snap_term = log_term
 *     (the ConfState is not in a record: the host fills it for the groups
 *     s_src names, as for qe_outbox's SNAP records); v_type = QE_VMSG_* with
 *     from, term, index, log_term and flags (0 with in->flags NULL).
 *  6. Class R.  Every wave member goes through Step's preamble with r.Term =
 *     f->term[g], in this order:
 *     a. term == 0 is a local message (raft/raft.go:850-851): it passes the
 *        term comparison (6d);
 *     b. term < r.Term: QE_ID_DROP_LOWER_TERM (:883-919: none of the response
 *        types is answered);
 *     c. term > r.Term: the lowest-position such member of the wave goes into
 *        the vote rows as v_type = QE_VMSG_VOTE_RESP with from, term, index and
 *        log_term 0 and flags QE_VMF_REJECT: QE_ID_STEPDOWN.  Every other such
 *        member is QE_ID_DEFERRED (a later pass drops it as not leading, once
 *        the term has risen);
 *     d. otherwise, f->state[g] != QE_STATE_LEADER: QE_ID_DROP_NOT_LEADER
 *        (stepFollower and stepCandidate have no arm for these messages);
 *        else QE_ID_ROUTED into the peer rows at [from*stride+g]: r_type =
 *        QE_MSG_* (type - 3), r_index = index, r_hint = hint, r_log_term =
 *        log_term and r_ctx = ctx (0 with in->ctx NULL; not written with r_ctx
 *        NULL).
 *  7. Consequences.  In one pass a group receives messages for ONE entry point;
 *     the one exception is an R wave that also yields one STEPDOWN vote row.
 *     Because of it the host calls qe_progress_step BEFORE qe_vote_step on the
 *     rows of one pass.  The preamble is evaluated at routing time and still
 *     holds at step time, because no other call of the pass touches the group.
 *     The same exception is the one case where qe_replies, listing the whole
 *     pass in one call, is inexact: the MsgTimeoutNow of such a group would
 *     carry the term the STEPDOWN row raised (qe_replies rule 5); a host that
 *     drives transfers lists timeout_now between the two calls.
 *  8. Rows.  f_type, s_type, v_type [G] and r_type (columns < G of each of the
 *     S slot rows; the pad columns are not touched) are COMPLETE: 0 where
 *     nothing was routed.  Every other row is written only where its type row
 *     is non-zero.  f_src / s_src / v_src [G] and r_src [S][stride] (each
 *     optional) get the list position of the routed record (v_src:
 *     QE_INBOX_SRC_TICK for the virtual HUP): the host copies payloads,
 *     ConfStates and heartbeat contexts by them.
 *  9. disposition[i] = QE_ID_* of every record.  deferred[0 .. *deferred_count)
 *     = the positions of the DEFERRED records, ascending; the next pass's list
 *     is those records followed by what arrived since.
 * 10. stats (optional): QE_STAT_GROUPS += groups with at least one record of
 *     disposition ROUTED; QE_STAT_INBOX_ROUTED / _STEPDOWN / _DEFERRED /
 *     _LOWER_TERM / _NOT_LEADER / _BAD += records by disposition, BAD also into
 *     QE_STAT_INVARIANT_VIOLATIONS; QE_STAT_CHECKSUM += mix64(mix64(group *
 *     0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03 ^ disposition << 56 ^ type << 48 ^
 *     from << 40) ^ i) per list record.
 * Every array is a DEVICE pointer; scratch is qe_inbox_scratch_bytes(G, S,
 * num_records) bytes of device memory, 8-B aligned: 4 * (3 + S) * G + n bytes
 * plus qe_collect_scratch_bytes(n) (0 for a num_slots outside 1..16).  It is
 * G-sized: see DESIGN.md.  Stream-ordered, no host synchronisation: an init
 * pass over the groups, three passes over the records, and qe_collect's count
 * and scan with a scatter of positions.  Positions are keys of 32-bit
 * atomicMin, which is order-free: the outputs are bit-exact from run to run.
 * QE_ERANGE: num_records > 0xFFFFFFF0.
 * QE_EINVAL: a NULL p / f / in / out; f->term or f->state NULL; num_slots
 * outside 1..16 or a nonzero reserved field of p; in->reserved nonzero;
 * stride < num_groups; msg_runs > QE_MAX_MSG_RUNS, or > 0 with a NULL
 * in->ent_len / in->ent_term / out->f_ent_len / out->f_ent_term; num_records
 * > 0 with a NULL group / from / type / term / index / log_term / commit /
 * hint (ctx, flags and tick_action may be NULL); a NULL row of qe_inbox_out
 * other than v_flags, r_ctx, f_ent_len / f_ent_term (msg_runs 0) and the four
 * *_src; scratch NULL (with num_groups > 0) or not 8-B aligned.  Every
 * argument check runs before the first HIP call.  num_records == 0 is QE_OK
 * with complete type rows (they may still hold tick HUPs) and *deferred_count
 * = 0; num_groups == 0 is QE_OK with *deferred_count = 0 and nothing else
 * written.
 *
 * With this call duties H4 and H6 of a host (tests/cluster_sim.py: Sim.deliver)
 * and the QE_TICK_HUP half of H1 are optional. */
#define QE_IMSG_APP 1                 /* MsgApp       (= QE_OMSG_APP)       */
#define QE_IMSG_SNAP 2                /* MsgSnap      (= QE_OMSG_SNAP)      */
#define QE_IMSG_HEARTBEAT 3           /* MsgHeartbeat (= QE_OMSG_HEARTBEAT) */
#define QE_IMSG_APP_RESP 4            /* QE_MSG_* + 3 ...                   */
#define QE_IMSG_APP_RESP_REJECT 5
#define QE_IMSG_HEARTBEAT_RESP 6
#define QE_IMSG_SNAP_STATUS 7
#define QE_IMSG_SNAP_STATUS_REJECT 8
#define QE_IMSG_UNREACHABLE 9
#define QE_IMSG_TRANSFER_LEADER 10
#define QE_IMSG_VOTE 11
#define QE_IMSG_PREVOTE 12
#define QE_IMSG_VOTE_RESP 13
#define QE_IMSG_PREVOTE_RESP 14
#define QE_IMSG_TIMEOUT_NOW 15
#define QE_IMSG_HUP 16                /* local MsgHup; `from` is not checked */
#define QE_ID_ROUTED 1            /* in this pass's rows                     */
#define QE_ID_STEPDOWN 2          /* a higher-term response, as a vote row   */
#define QE_ID_DEFERRED 3          /* waits for the next pass                 */
#define QE_ID_DROP_LOWER_TERM 4
#define QE_ID_DROP_NOT_LEADER 5
#define QE_ID_BAD 255
#define QE_INBOX_SRC_TICK 0xFFFFFFFFu /* v_src of the virtual HUP            */
#define QE_STAT_INBOX_ROUTED QE_STAT_VOTE_WON        /* qe_inbox: records by disposition */
#define QE_STAT_INBOX_STEPDOWN QE_STAT_STEPDOWNS
#define QE_STAT_INBOX_DEFERRED QE_STAT_VOTE_PENDING
#define QE_STAT_INBOX_LOWER_TERM QE_STAT_VOTE_LOST
#define QE_STAT_INBOX_NOT_LEADER QE_STAT_REJECTED
#define QE_STAT_INBOX_BAD QE_STAT_COMMIT_INF

typedef struct qe_inbox_in {
  uint64_t num_records;         /* n <= 0xFFFFFFF0 */
  uint32_t msg_runs;            /* E, 0..QE_MAX_MSG_RUNS */
  uint32_t reserved;            /* must be 0 */
  const uint64_t *group;        /* [n] the RECEIVER's global group id */
  const uint8_t  *from, *type;  /* [n] the sender's slot in the receiver's numbering, QE_IMSG_* */
  const uint64_t *term, *index, *log_term, *commit;  /* [n]; index / log_term are also
                                   Metadata.Index / Term of a MsgSnap */
  const uint64_t *hint;         /* [n] m.RejectHint */
  const uint32_t *ctx;          /* [n] or NULL: the context number of a MsgHeartbeatResp */
  const uint8_t  *flags;        /* [n] or NULL: QE_VMF_* */
  const uint32_t *ent_len;      /* [E][n] */
  const uint64_t *ent_term;     /* [E][n] */
  const uint8_t  *tick_action;  /* [G] or NULL: qe_tick's action row (QE_TICK_HUP is read) */
} qe_inbox_in;

typedef struct qe_inbox_out {
  uint8_t  *f_type, *f_from;    /* [G] qe_leader_msgs */
  uint64_t *f_term, *f_index, *f_log_term, *f_commit;
  uint32_t *f_ent_len;          /* [E][stride] */
  uint64_t *f_ent_term;         /* [E][stride] */
  uint8_t  *s_type, *s_from;    /* [G] qe_snap_msgs */
  uint64_t *s_term, *s_snap_index, *s_snap_term;
  uint8_t  *v_type, *v_from;    /* [G] qe_vote_msgs */
  uint64_t *v_term, *v_index, *v_log_term;
  uint8_t  *v_flags;            /* [G] or NULL */
  uint8_t  *r_type;             /* [S][stride] qe_peer_msgs */
  uint64_t *r_index, *r_hint, *r_log_term;
  uint32_t *r_ctx;              /* [S][stride] or NULL */
  uint32_t *f_src, *s_src, *v_src;  /* [G], each or NULL */
  uint32_t *r_src;              /* [S][stride] or NULL */
  uint8_t  *disposition;        /* [n] QE_ID_* */
  uint32_t *deferred;           /* [n] positions of the DEFERRED records, ascending */
  uint64_t *deferred_count;     /* device */
} qe_inbox_out;

size_t qe_inbox_scratch_bytes(uint64_t num_groups, uint32_t num_slots, uint64_t num_records);
int qe_inbox(const qe_progress *p, const qe_follower *f, const qe_inbox_in *in,
             const qe_inbox_out *out, void *scratch, uint64_t *stats, void *stream);

/* qe_replies (additive in ABI 8): the messages the RECEIVER-side calls sent,
 * as a dense, ordered list of records on the device, in the record layout
 * qe_inbox consumes (QE_IMSG_* types) -- the half of Ready.Messages that
 * qe_outbox does not list.  qe_follower_step, qe_snapshot_step and
 * qe_vote_step report a send as a result code and a few rows, qe_progress_step
 * its MsgTimeoutNow as a mask; this call turns them into MsgAppResp /
 * MsgHeartbeatResp, Msg{Pre}VoteResp, Msg{Pre}Vote and MsgTimeoutNow records.
 * With qe_outbox and qe_inbox the loop tick -> step -> (outbox + replies) ->
 * transport -> inbox -> step moves no G-sized row to the host in either
 * direction; where the receivers share the batch, qe_carry is that transport
 * and no record leaves the device.  It writes nothing resident.  Of p it reads num_groups (G),
 * group_offset, num_slots (S), stride and, when the V family is given,
 * last_index, and nothing else.  A family is present iff its result row is
 * non-NULL; full = (1 << S) - 1.
 *
 *  1. Kinds, in this order per group:
 *     F response, f_result[g] one of
 *       QE_FR_LOWER_TERM_RESP: QE_IMSG_APP_RESP with index 0 (the empty
 *         MsgAppResp of raft/raft.go:906);
 *       QE_FR_HEARTBEAT_RESP: QE_IMSG_HEARTBEAT_RESP with ctx = f_ctx[g], 0 with
 *         f_ctx NULL (handleHeartbeat echoes m.Context, :1515);
 *       QE_FR_APP_ACCEPT / QE_FR_APP_STALE: QE_IMSG_APP_RESP with index =
 *         f_resp_index[g] (:1482, :1477);
 *       QE_FR_APP_REJECT: QE_IMSG_APP_RESP_REJECT with index = f_resp_index[g],
 *         hint = f_reject_hint[g], log_term = f_resp_log_term[g] (:1502-1509);
 *       each with to = f_from[g] and term = in->term[g].
 *     S response, s_result[g] one of QE_SR_STALE, QE_SR_NOT_MEMBER,
 *       QE_SR_FAST_FORWARD, QE_SR_RESTORED: QE_IMSG_APP_RESP with index =
 *       s_resp_index[g], to = s_from[g], term = in->term[g] (:1523, :1527).
 *     V response, v_result[g] QE_VR_GRANT or QE_VR_REJECT: QE_IMSG_VOTE_RESP
 *       for v_type[g] == QE_VMSG_VOTE, QE_IMSG_PREVOTE_RESP for QE_VMSG_PREVOTE
 *       (voteRespMsgType), QE_RMSG_BAD for any other v_type; to = v_from[g],
 *       term = v_resp_term[g], flags = QE_VMF_REJECT for a REJECT (:968, :977,
 *       :913).
 *     V request, v_result[g] QE_VR_CAMPAIGN_VOTE or QE_VR_CAMPAIGN_PREVOTE: one
 *       QE_IMSG_VOTE / QE_IMSG_PREVOTE to every set bit of v_req_to[g] & full,
 *       with term = v_resp_term[g], index = p->last_index[g], log_term =
 *       v_req_log_term[g] (:833), and flags = QE_VMF_FORCE where v_type[g] ==
 *       QE_VMSG_TIMEOUT_NOW and the result is CAMPAIGN_VOTE: the
 *       campaignTransfer context (:818-835).
 *     T, one QE_IMSG_TIMEOUT_NOW to every set bit of timeout_now[g] & full,
 *       with term = in->term[g] (sendTimeoutNow, :1722-1724).
 *     Every other result code, every refused result (>= 16) and every absent
 *     family yields nothing.  A field a kind does not name is 0.  group =
 *     group_offset + g: the SENDER.
 *  2. BAD.  A single-`to` record (F, S, V response) whose to >= num_slots gets
 *     type QE_RMSG_BAD, as does the V response whose v_type is no request.  It
 *     keeps group, to and term as computed; every other field is 0.  *count
 *     depends on the result rows and the masks alone, never on a from / type row.
 *  3. Order.  Records are listed by ascending tile (g / 64), then kind (F, S, V
 *     response, V request, T); within the three single-record kinds then g,
 *     within the two mask kinds then slot, then g: qe_outbox's order with the
 *     kind in front of the slot.  The order is part of the contract.
 *  4. Truncation, as qe_outbox: a record at a position >= capacity is not
 *     written; *count is still the full number, and nothing at or past
 *     min(*count, capacity) is touched in any output array.
 *  5. The term row.  in->term is qe_follower.term as it stands when qe_replies
 *     runs: a call lists the outputs of the step calls made since that row
 *     last changed for the groups concerned (F, S and T records carry the
 *     receiver's term after its step; V records carry v_resp_term).  Listing a
 *     whole qe_inbox pass in one call is inexact in ONE case (qe_inbox rule 7):
 *     a group whose R wave set a timeout_now bit in qe_progress_step and whose
 *     STEPDOWN vote row then raised the term in qe_vote_step of the same pass.
 *     Its MsgTimeoutNow would carry the new term, where r.send (:415) stamps
 *     the term of the leader that sent it.  A host that drives leadership
 *     transfers lists timeout_now in a call of its own, between
 *     qe_progress_step and qe_vote_step.
 *  6. stats (optional), over every record asked for, those past capacity too:
 *     QE_STAT_GROUPS += groups with at least one record;
 *     QE_STAT_REPLY_APP_RESP / _HEARTBEAT_RESP / _VOTE_RESP / _VOTE_REQ /
 *     _TIMEOUT_NOW / _BAD += records by type (APP_RESP: accept, stale, lower
 *     term, snapshot and reject records; a BAD record counts as BAD alone), BAD
 *     also into QE_STAT_INVARIANT_VIOLATIONS; QE_STAT_CHECKSUM += h6 per record,
 *     h1 = mix64(group * 0x9E3779B97F4A7C15 ^ 0xA0761D6478BD642F ^ type << 56 ^
 *     to << 48), h2 = mix64(h1 ^ term), h3 = mix64(h2 ^ index), h4 = mix64(h3 ^
 *     log_term), h5 = mix64(h4 ^ hint), h6 = mix64(h5 ^ (ctx | (uint64)flags <<
 *     32)), the fields as the record holds them (ctx and flags too where their
 *     arrays are NULL).
 * `count` and every array of both structs are DEVICE pointers; scratch is
 * qe_replies_scratch_bytes(num_groups) (== qe_collect_scratch_bytes) bytes of
 * device memory, 8-B aligned.  Stream-ordered: three kernels (count per
 * 4096-group chunk, the scan of qe_collect, fill), no host synchronisation.
 * QE_EINVAL: a NULL p / in / out / count / term; scratch NULL (with num_groups
 * > 0) or not 8-B aligned; num_slots outside 1..16; a nonzero reserved field
 * of p or in; stride < num_groups; f_result without f_from, f_resp_index,
 * f_reject_hint or f_resp_log_term; s_result without s_from or s_resp_index;
 * v_result without v_type, v_from, v_resp_term, v_req_log_term, v_req_to or
 * p->last_index; capacity > 0 with a NULL group / to / type / term / index /
 * log_term / hint array (ctx and flags may be NULL: not written).  Every
 * argument check runs before the first HIP call.  num_groups == 0 is QE_OK
 * with *count = 0, and so is a call with every family absent.
 *
 * With this call duty H8 of a host (tests/cluster_sim.py), the vote half of H4
 * and the MsgTimeoutNow of a transfer are optional: the host copies
 * min(*count, capacity) records instead of the G-sized result rows it would
 * walk.  MsgSnapStatus (H11) is reported by what carries the MsgSnap: qe_carry
 * for a receiver in the batch, the host's transport otherwise. */
#define QE_RMSG_BAD 255      /* a response whose `to` is no slot, or a GRANT / REJECT
                                whose message type is no request */
#define QE_STAT_REPLY_APP_RESP QE_STAT_VOTE_WON            /* qe_replies: records by type */
#define QE_STAT_REPLY_HEARTBEAT_RESP QE_STAT_VOTE_PENDING
#define QE_STAT_REPLY_VOTE_RESP QE_STAT_GRANTED
#define QE_STAT_REPLY_VOTE_REQ QE_STAT_ELECTIONS
#define QE_STAT_REPLY_TIMEOUT_NOW QE_STAT_LEADERS
#define QE_STAT_REPLY_BAD QE_STAT_REJECTED

typedef struct qe_replies_in {
  const uint64_t *term;          /* [G] required: qe_follower.term as it stands AFTER the listed calls */
  /* F: qe_follower_step (family present iff f_result != NULL) */
  const uint8_t  *f_result;      /* [G] qe_follower_out.result */
  const uint8_t  *f_from;        /* [G] qe_leader_msgs.from */
  const uint64_t *f_resp_index, *f_reject_hint, *f_resp_log_term;   /* [G] */
  const uint32_t *f_ctx;         /* [G] or NULL: the context the heartbeat carried (echoed) */
  /* S: qe_snapshot_step (present iff s_result != NULL) */
  const uint8_t  *s_result, *s_from;   /* [G] */
  const uint64_t *s_resp_index;        /* [G] */
  /* V: qe_vote_step (present iff v_result != NULL) */
  const uint8_t  *v_result, *v_type, *v_from;   /* [G] qe_vote_out.result, qe_vote_msgs.type / from */
  const uint64_t *v_resp_term, *v_req_log_term; /* [G] */
  const void     *v_req_to;      /* [G] mask-typed */
  /* T: qe_progress_step */
  const void     *timeout_now;   /* [G] mask-typed or NULL */
  uint32_t reserved[2];          /* must be 0 */
} qe_replies_in;

typedef struct qe_replies_out {
  uint64_t capacity;
  uint64_t *group;               /* [capacity] group_offset + g (the SENDER) */
  uint8_t  *to, *type;           /* [capacity] slot, QE_IMSG_* or QE_RMSG_BAD */
  uint64_t *term, *index, *log_term, *hint;   /* [capacity] */
  uint32_t *ctx;                 /* [capacity] or NULL */
  uint8_t  *flags;               /* [capacity] or NULL: QE_VMF_* */
  uint64_t *count;               /* device: records asked for (may exceed capacity) */
} qe_replies_out;

size_t qe_replies_scratch_bytes(uint64_t num_groups);   /* == qe_collect_scratch_bytes */
int qe_replies(const qe_progress *p, const qe_replies_in *in, const qe_replies_out *out,
               void *scratch, uint64_t *stats, void *stream);

/* qe_carry (additive in ABI 8): a list of sent records -- a qe_outbox_out or a
 * qe_replies_out list as it stands, `group` the sender and `to` a slot in the
 * sender's numbering -- turned into the list the receivers' qe_inbox reads,
 * `group` the receiver and `from` the sender's slot in the receiver's
 * numbering.  It is the in-process `network` of the reference's tests
 * (raft/raft_test.go:4633-4778): send maps m.To to a peer, filter (:4750-4774)
 * drops by message type (ignorem), by directed link (dropm, cut, isolate) and by
 * hook, and panics on a MsgHup.  Where the replicas of a group are co-resident
 * in one batch, the loop step -> outbox / replies -> carry -> inbox -> step
 * never leaves the device.  The mapping is the host's table, qe_peers: slot
 * assignment stays with the host.  Of p the call reads num_groups (G),
 * group_offset, num_slots (S) and stride and nothing else; it writes nothing
 * resident.  n = min(*in->count, in->capacity) is read on the device, as
 * qe_advance reads a list's length; the launches are sized by in->capacity.
 *
 * Per source record i < n, with g = group[i] - group_offset, in this order:
 *  1. QE_TD_BAD.  type[i] outside {1..6, 10..15} (0, the local
 *     QE_IMSG_SNAP_STATUS / _SNAP_STATUS_REJECT / _UNREACHABLE, QE_IMSG_HUP --
 *     the reference's panic in filter -- and above, QE_OMSG_BAD / QE_RMSG_BAD
 *     included); g >= G; to[i] >= S; peer_group[to*stride+g] == QE_PEER_NONE;
 *     or the receiver is in the batch and peer_from[to*stride+g] >= S.  A BAD
 *     record yields nothing.
 *  2. QE_TD_LOST.  Bit type[i] of `ignore` is set, or drop[i] != 0, or bit
 *     to[i] of cut[g] is set.  Only the SENDER's link bit is read: a two-way cut
 *     is two bits, as network.cut is two drops.  A LOST record yields no
 *     carried record.
 *  3. QE_TD_REMOTE.  The receiver's id peer_group[to*stride+g] is outside
 *     [group_offset, group_offset + G).  i goes into `remote`; nothing goes into
 *     the local list and no status record: the transport that really carries
 *     the record reports it.
 *  4. QE_TD_LOCAL.  One local record: group = peer_group[to*stride+g], from =
 *     peer_from[to*stride+g]; type, term, index, log_term, commit, hint, ctx and
 *     mflags copied (0 where the source array is NULL); the ent rows j <
 *     in->msg_runs copied, the rows in->msg_runs <= j < out->msg_runs 0.
 *  5. MsgSnapStatus (duty H11; node.ReportSnapshot, raft/raft.go:1310-1331),
 *     with QE_CARRY_SNAP_STATUS in in->flags.  A QE_IMSG_SNAP record that is
 *     LOCAL is followed directly by a local record with group = group[i] (the
 *     sender), from = to[i], type = QE_IMSG_SNAP_STATUS and term (a local
 *     message) and every other field 0.  A QE_IMSG_SNAP record that is LOST
 *     (wherever its receiver lives: the loss was decided here) yields that
 *     record alone, with QE_IMSG_SNAP_STATUS_REJECT.  So a source record yields
 *     0, 1 or 2 local records.
 *  6. Order and truncation.  The local list is in source order, a status record
 *     directly behind its MsgSnap; local record k goes to position base + k of
 *     the qe_carry_out arrays, its ent rows to [j*ent_pitch + base + k].  A
 *     local record at a position >= out->capacity is not written; *out->count
 *     is still the full number of local records (it does not include base),
 *     and nothing below base or at or past min(base + *count, capacity) is
 *     touched.  src[k] (optional) = i, for a status record the i of its MsgSnap.
 *     disposition[i] = QE_TD_* for i < n and is not touched at or past n;
 *     remote[0 .. *remote_count) = the positions of the REMOTE records,
 *     ascending.  Two calls chain: the second takes base = base + *count of the
 *     first (read back once, or known from the capacities).
 *  7. stats (optional): QE_STAT_CARRY_LOCAL / _REMOTE / _LOST / _BAD += source
 *     records by disposition, BAD also into QE_STAT_INVARIANT_VIOLATIONS;
 *     QE_STAT_CARRY_SNAP_STATUS += status records (both kinds); QE_STAT_GROUPS
 *     += local records ASKED FOR (*out->count: those past capacity too);
 *     QE_STAT_CHECKSUM += mix64(mix64(group[i] * 0x9E3779B97F4A7C15 ^
 *     0x8CB92BA72F3D8DD7 ^ disposition << 56 ^ type << 48 ^ to << 40) ^ i) per
 *     source record i < n.
 * Every array, count included, is a DEVICE pointer; `cut` is mask-typed
 * (qe_mask_bytes(S) bytes per group).  scratch is
 * qe_carry_scratch_bytes(in->capacity) bytes of device memory, 8-B aligned: two
 * bytes per record plus 2 * qe_collect_scratch_bytes(capacity).  Nothing in it
 * is G-sized.  Stream-ordered, no host synchronisation: a classify pass, the
 * count and scan of each of the two lists, the fill of the local list and the
 * scatter of the remote positions.  No atomics but the statistics: the outputs
 * are bit-exact from run to run.
 * QE_ERANGE: in->capacity > 0xFFFFFFF0 (positions are 32-bit).
 * QE_EINVAL: a NULL p / peers / in / out; num_slots outside 1..16 or a nonzero
 * reserved field of p, in or out; stride < num_groups; a NULL peer_group /
 * peer_from / in->count / out->count / out->remote_count; in->capacity > 0
 * with a NULL in->group / to / type / term / index / log_term (commit, hint,
 * ctx, mflags, drop and cut may be NULL), a NULL out->disposition / remote, or
 * a NULL scratch; scratch not 8-B aligned; in->msg_runs > out->msg_runs or
 * either > QE_MAX_MSG_RUNS; in->msg_runs > 0 with a NULL in->ent_len /
 * ent_term; base > out->capacity; out->capacity > 0 with a NULL out->group /
 * from / type / term / index / log_term / commit / hint (ctx, mflags and src may
 * be NULL: not written) or, with out->msg_runs > 0, a NULL out->ent_len /
 * ent_term or ent_pitch < capacity; `ignore` with a bit outside the carriable
 * types {1..6, 10..15}; `flags` other than QE_CARRY_SNAP_STATUS.  Every
 * argument check runs before the first HIP call.  in->capacity == 0 is QE_OK
 * with *out->count = *out->remote_count = 0.
 *
 * With this call duty H11 of a host (tests/cluster_sim.py: Sim.snap_status) and
 * the addressing half of Sim.send are optional for co-resident replicas.
 * Duplication and delay are a schedule, the host's or the simulation's. */
#define QE_PEER_NONE 0xFFFFFFFFFFFFFFFFull   /* no peer behind this slot */
#define QE_CARRY_SNAP_STATUS 1u   /* in->flags: rule 5 */
#define QE_CARRY_TYPES 0x0000FC7Eu /* the carriable types, as `ignore` bits */
#define QE_TD_LOCAL 1             /* in the local list                        */
#define QE_TD_REMOTE 2            /* the receiver is outside the batch        */
#define QE_TD_LOST 3              /* ignorem / drop / cut                     */
#define QE_TD_BAD 255
#define QE_STAT_CARRY_LOCAL QE_STAT_VOTE_WON          /* qe_carry: records by disposition */
#define QE_STAT_CARRY_LOST QE_STAT_VOTE_LOST
#define QE_STAT_CARRY_REMOTE QE_STAT_VOTE_PENDING
#define QE_STAT_CARRY_BAD QE_STAT_COMMIT_INF
#define QE_STAT_CARRY_SNAP_STATUS QE_STAT_COMMIT_ADVANCED  /* ... status records made */

typedef struct qe_peers {            /* resident, the host's slot assignment */
  const uint64_t *peer_group;        /* [S][stride] global id of the group that is the peer in slot s of g */
  const uint8_t  *peer_from;         /* [S][stride] g's slot in that group's numbering */
} qe_peers;

typedef struct qe_carry_in {         /* a qe_outbox_out or qe_replies_out list, as it stands */
  uint64_t capacity;                 /* records the arrays hold; ent pitch */
  const uint64_t *count;             /* DEVICE: n = min(*count, capacity), as qe_advance takes a list */
  uint32_t msg_runs;                 /* E_in, 0..QE_MAX_MSG_RUNS */
  uint32_t flags;                    /* QE_CARRY_SNAP_STATUS */
  const uint64_t *group; const uint8_t *to, *type;
  const uint64_t *term, *index, *log_term;
  const uint64_t *commit;            /* or NULL = 0 (a replies list) */
  const uint64_t *hint;              /* or NULL = 0 (an outbox list) */
  const uint32_t *ctx; const uint8_t *mflags;   /* each or NULL = 0 */
  const uint32_t *ent_len; const uint64_t *ent_term;  /* [E_in][capacity] */
  const uint8_t  *drop;              /* [capacity] or NULL: nonzero = this record is lost (msgHook / a fractional dropm draw, the host's) */
  const void     *cut;               /* [G] mask-typed or NULL: bit s of cut[g] = the link g -> slot s is down (dropm >= 1) */
  uint32_t ignore;                   /* bit t set: records of type t are lost (ignorem) */
  uint32_t reserved;                 /* must be 0 */
} qe_carry_in;

typedef struct qe_carry_out {        /* the local list is in qe_inbox_in's layout */
  uint64_t capacity, base, ent_pitch; /* local record k goes to position base + k; ent rows at [j*ent_pitch + base + k] */
  uint32_t msg_runs, reserved;       /* E_out >= E_in */
  uint64_t *group; uint8_t *from, *type;
  uint64_t *term, *index, *log_term, *commit, *hint;
  uint32_t *ctx; uint8_t *mflags;    /* each or NULL: not written */
  uint32_t *ent_len; uint64_t *ent_term;
  uint32_t *src;                     /* or NULL: the source position of local record k (a status record: its MsgSnap's) */
  uint64_t *count;                   /* DEVICE: local records asked for (may exceed capacity - base) */
  uint8_t  *disposition;             /* [in.capacity] QE_TD_* for i < n */
  uint32_t *remote;                  /* [in.capacity] positions of the REMOTE records, ascending */
  uint64_t *remote_count;            /* DEVICE */
} qe_carry_out;

size_t qe_carry_scratch_bytes(uint64_t capacity);
int qe_carry(const qe_progress *p, const qe_peers *peers, const qe_carry_in *in,
             const qe_carry_out *out, void *scratch, uint64_t *stats, void *stream);

/* qe_ready_note / qe_ready / qe_advance (additive in ABI 8): the storage half
 * of RawNode.Ready() as a dense device list, and the Advance() that moves the
 * cursors -- the half of a Ready that qe_outbox / qe_replies (Messages) do not
 * list: the HardState and SoftState deltas, the entries to persist, the
 * entries to apply, a pending snapshot and MustSync (raft/rawnode.go:133-179,
 * raft/node.go:562-593, raft/log.go:170-197, raft/log_unstable.go).  A host
 * asks "which groups have something to persist or apply, and what?" and copies
 * min(*count, capacity) records instead of the G-sized term, vote, commit,
 * lead, state and last_index rows.
 *
 * qe_ready_state, eight resident rows [G], read-write, device:
 *   stable        unstable.offset - 1: every entry <= stable is in Storage
 *   applied       raftLog.applied (the row qe_propose / qe_compact read)
 *   snap_pending  index of unstable.snapshot, 0 = none
 *   prev_term, prev_commit, prev_vote   rn.prevHardSt (vote as a slot, >=
 *                 num_slots = None)
 *   prev_lead, prev_state               rn.prevSoftSt (lead as a slot)
 * NewRawNode: prev := current, stable = last_index, snap_pending = 0; applied
 * is the caller's.  In every rule below a vote or lead >= num_slots is None,
 * whatever its value: two different encodings of None are equal.
 *
 * qe_ready_note keeps unstable.offset right across receiver steps: it runs
 * after a qe_follower_step and / or a qe_snapshot_step, on their own result
 * rows (each pair of rows optional; of p it reads num_groups alone).
 *   follow_result[g] == QE_FR_APP_ACCEPT && append_from[g] != 0:
 *     stable = min(stable, append_from - 1) (unstable.truncateAndAppend,
 *     log_unstable.go:121-141: only its `after <= offset` arm moves offset);
 *   then snap_result[g] == QE_SR_RESTORED: stable = snap_pending =
 *     snap_resp_index[g] (unstable.restore, :115-119).
 * Leader-side appends (qe_propose, qe_become_leader) never truncate and need
 * no note.  QE_EINVAL: a NULL p / rs / in / stable; one row of a pair without
 * the other; snap_result with a NULL snap_pending.
 *
 * qe_ready: HasReady + readyWithoutAccept over the batch.  Of p it reads
 * num_groups (G), group_offset, num_slots (S), stride, log_runs, committed,
 * last_index, run_first, run_term, run_count; of f term, state, lead, vote (a
 * NULL vote row: None everywhere); the rows of rs; in->pending.  It writes
 * nothing resident.  Per group g:
 *  1. hard = (term, vote, committed); hard_changed = hard != (prev_term,
 *     prev_vote, prev_commit); hard_empty = term 0, vote None, committed 0.
 *     soft = (lead, state); soft_changed = soft != (prev_lead, prev_state).
 *  2. Entries = (stable, last_index]: ent_first = stable + 1 (in every
 *     record).  With ent_runs E > 0 they are cut into the table's term runs
 *     exactly as qe_outbox rule 4 cuts a MsgApp with index = stable and
 *     max_entries 0, its cap of 0xFFFFFFFF entries included: the range listed
 *     is (stable, min(last_index, stable + 0xFFFFFFFF)], so every ent_len fits
 *     its uint32.  Run j is
 *     the j-th table run that overlaps the range, ent_len[j*capacity+i] its
 *     overlap, ent_term[j*capacity+i] its term; the list ends after E runs and
 *     QE_RD_ENTS_CUT is set when it ends below last_index.  ent_count = the
 *     entries listed, ent_last_term = the term of the last listed entry (what
 *     stableTo needs), 0 with none.  With E = 0 no runs are listed and the
 *     range is whole: ent_count = last_index - stable, ent_last_term =
 *     term(last_index).  The caller keeps run_first[0] <= stable (results are
 *     unspecified otherwise; memory stays in bounds).
 *  3. CommittedEntries (raftLog.nextEnts): off = max(applied + 1, run_first[0]
 *     + 1); if committed + 1 > off they are [off, hi], hi = committed, or off +
 *     max_apply - 1 when max_apply is nonzero and smaller (the entry-count
 *     model of maxNextEntsSize, as max_ents models MaxSizePerMsg).  With E > 0
 *     they are cut into term runs as the entries are, 0xFFFFFFFF entries from
 *     off at most (apply_len / apply_term,
 *     a second [E][capacity] pair) and end after E runs.  apply_count = the
 *     entries listed, apply_first = off (0 with apply_count 0);
 *     QE_RD_APPLY_CUT is set when the list ends below committed.
 *  4. Snapshot: snap_pending != 0 -> QE_RD_SNAP, snap_index = snap_pending.
 *  5. MustSync (node.go:586-593) = Entries non-empty || vote != prev_vote ||
 *     term != prev_term -> QE_RD_MUST_SYNC.
 *  6. Listing.  g is listed iff soft_changed, or !hard_empty && hard_changed,
 *     or snap_pending != 0, or Entries is non-empty, or CommittedEntries is
 *     non-empty, or pending[g] != 0 (an optional row for what this call
 *     cannot see: messages, which qe_outbox / qe_replies list, and
 *     ReadStates, which qe_read_states lists).
 *  7. Every listed record: group = group_offset + g, term, commit =
 *     committed, vote and lead (0xFF for None), state, and flags: QE_RD_SOFT
 *     where soft_changed, QE_RD_HARD where !hard_empty && hard_changed (only
 *     then does a Ready carry the HardState), MUST_SYNC, SNAP and the two CUT
 *     bits.  Unused run rows of a record are 0.
 *  8. Order and truncation.  Records are listed by ascending g; *count is the
 *     full number; nothing at or past min(*count, capacity) is touched in any
 *     output array (qe_outbox rule 3).
 *  9. stats (optional), over every listed group, those past capacity too:
 *     QE_STAT_GROUPS += records; QE_STAT_READY_ENTRIES += ent_count;
 *     QE_STAT_READY_APPLY += apply_count; QE_STAT_READY_MUST_SYNC += MustSync
 *     records; QE_STAT_CHECKSUM += h9 per record, h1 = mix64(group *
 *     0x9E3779B97F4A7C15 ^ 0x8CB92BA72F3D8DD7 ^ flags << 56 ^ vote << 48 ^ lead
 *     << 40 ^ state << 32), then hk = mix64(hk-1 ^ x) over x = term, commit,
 *     ent_first, ent_count, ent_last_term, apply_first, apply_count,
 *     snap_index, as the record holds them.
 * `count` and every array of qe_ready_out are DEVICE pointers; scratch is
 * qe_ready_scratch_bytes(num_groups) bytes of device memory, 8-B aligned (the
 * chunk offsets and counts of qe_collect and one flag byte per group).
 * Stream-ordered: three kernels (count: one wave per 4096-group chunk, the
 * scan of qe_collect, fill), no host synchronisation.
 * QE_EINVAL: a NULL p / f / rs / in / out / count / scratch (with num_groups >
 * 0); a NULL term, state or lead; a NULL committed, last_index, run_first,
 * run_term or run_count; a NULL row of rs; stride < num_groups; num_slots
 * outside 1..16; log_runs 0 or > QE_MAX_LOG_RUNS; ent_runs > QE_MAX_MSG_RUNS,
 * or > 0 without ent_len / ent_term / apply_len / apply_term; capacity > 0
 * with a NULL field array (group, term, commit, vote, lead, state, flags,
 * ent_first, ent_count, ent_last_term, apply_first, apply_count, snap_index);
 * a nonzero reserved field; scratch not 8-B aligned.  Every argument check
 * runs before the first HIP call.  num_groups == 0 is QE_OK with *count = 0.
 *
 * qe_advance: acceptReady + RawNode.Advance + raft.advance (rawnode.go:
 * 140-179, raft.go:543-580), driven by a record list in qe_ready's layout:
 * `list` with its capacity, arrays and device count; n = min(*count,
 * capacity) records, one thread each, so the work is n-sized, not G-sized.
 * The run rows of the list are not read.  result[i] per record:
 *  1. group - group_offset outside [0, G): QE_ADV_BAD_GROUP, nothing written.
 *  2. newApplied = apply_first + apply_count - 1 when apply_count > 0, else
 *     snap_index under QE_RD_SNAP, else 0 (Ready.appliedCursor).  newApplied >
 *     0 and (committed < newApplied or newApplied < applied) is appliedTo's
 *     panic: QE_ADV_APPLIED_RANGE, nothing of the group is written.  Otherwise
 *     applied = newApplied (when > 0).
 *  3. QE_RD_HARD: prev_term, prev_vote, prev_commit take the record's values.
 *     QE_RD_SOFT: prev_lead, prev_state take the record's.
 *  4. ent_count > 0: stableTo(i = ent_first + ent_count - 1, ent_last_term)
 *     moves stable = i only when stable < i <= last_index and term(i) on the
 *     run table equals ent_last_term; otherwise the outcome is
 *     QE_ADV_OK_STALE_ENTRIES: the log was truncated under the Ready, and the
 *     next qe_ready lists the entries again.
 *  5. QE_RD_SNAP and snap_pending == snap_index: snap_pending = 0
 *     (stableSnapTo).
 *  6. With auto_leave (and then pending_conf_index and f->state, all [G]):
 *     QE_ADV_AUTO_LEAVE is set in the result where newApplied > 0, auto_leave[g]
 *     != 0, f->state[g] == QE_STATE_LEADER and applied-before <=
 *     pending_conf_index[g] <= newApplied (raft.go:554).  The append itself
 *     stays the caller's qe_propose with QE_PROP_APPEND_ONLY.
 * result & QE_ADV_OUTCOME is QE_ADV_OK, _OK_STALE_ENTRIES, or a refusal (>=
 * QE_ADV_REFUSED).  A group listed twice in one list is unspecified (memory
 * stays in bounds); qe_ready never does it.  reduceUncommittedSize stays with
 * the host, as for qe_propose.
 * Of p it reads num_groups, group_offset, stride, log_runs, committed,
 * last_index, run_first, run_term, run_count.  QE_EINVAL: a NULL p / rs / list
 * / list->count / result; a NULL row of rs; a NULL log row of p; stride <
 * num_groups; log_runs out of range; capacity > 0 with a NULL field array (as
 * qe_ready's); a nonzero reserved field; auto_leave without
 * pending_conf_index or f->state.  capacity == 0 or num_groups == 0 is QE_OK:
 * nothing is written.
 *
 * DIVERGENCE from the reference: acceptReady is folded into qe_advance.
 * RawNode.Ready() moves prevSoftSt at once; here a second qe_ready before the
 * qe_advance lists the same SoftState again.
 *
 * With these calls the unstable / applied bookkeeping of a host (tests/
 * trace_cluster.py Replay.ready / appended) is optional. */
#define QE_RD_SOFT 1u        /* the record's lead / state are a SoftState delta */
#define QE_RD_HARD 2u        /* the record's term / vote / commit are a HardState delta */
#define QE_RD_MUST_SYNC 4u
#define QE_RD_SNAP 8u        /* snap_index: the snapshot to persist and apply */
#define QE_RD_ENTS_CUT 16u   /* the entries list ends below last_index */
#define QE_RD_APPLY_CUT 32u  /* the apply list ends below committed */
#define QE_ADV_OK 1
#define QE_ADV_OK_STALE_ENTRIES 2
#define QE_ADV_REFUSED 8          /* outcomes >= this: nothing of the group changed */
#define QE_ADV_BAD_GROUP 8
#define QE_ADV_APPLIED_RANGE 9
#define QE_ADV_OUTCOME 0x0Fu
#define QE_ADV_AUTO_LEAVE 0x10u   /* result bit: the leader appends the leave-joint entry */
#define QE_STAT_READY_ENTRIES QE_STAT_COMMIT_SUM      /* qe_ready: entries listed */
#define QE_STAT_READY_APPLY QE_STAT_COMMIT_ADVANCED   /* ... entries to apply */
#define QE_STAT_READY_MUST_SYNC QE_STAT_VOTE_WON      /* ... records with MustSync */

typedef struct qe_ready_state {
  uint64_t *stable;               /* [G] rw */
  uint64_t *applied;              /* [G] rw */
  uint64_t *snap_pending;         /* [G] rw */
  uint64_t *prev_term, *prev_commit;          /* [G] rw */
  uint8_t  *prev_vote, *prev_lead, *prev_state; /* [G] rw */
} qe_ready_state;

typedef struct qe_ready_note_in {
  const uint8_t  *follow_result;   /* [G] or NULL: qe_follower_out.result */
  const uint64_t *append_from;     /* [G], with follow_result */
  const uint8_t  *snap_result;     /* [G] or NULL: qe_snap_out.result */
  const uint64_t *snap_resp_index; /* [G], with snap_result */
} qe_ready_note_in;

typedef struct qe_ready_in {
  const uint8_t *pending;         /* [G] or NULL */
  uint32_t max_apply;             /* entries to apply per record at most, 0 = no limit */
  uint32_t reserved;              /* must be 0 */
} qe_ready_in;

typedef struct qe_ready_out {
  uint64_t capacity;              /* records the arrays hold */
  uint32_t ent_runs;              /* E, 0..QE_MAX_MSG_RUNS */
  uint32_t reserved;
  uint64_t *group;                /* [capacity] group_offset + g */
  uint64_t *term, *commit;        /* [capacity] */
  uint8_t  *vote, *lead, *state;  /* [capacity] */
  uint8_t  *flags;                /* [capacity] QE_RD_* */
  uint64_t *ent_first, *ent_count, *ent_last_term;   /* [capacity] */
  uint64_t *apply_first, *apply_count;               /* [capacity] */
  uint64_t *snap_index;           /* [capacity] */
  uint32_t *ent_len;              /* [E][capacity] */
  uint64_t *ent_term;             /* [E][capacity] */
  uint32_t *apply_len;            /* [E][capacity] */
  uint64_t *apply_term;           /* [E][capacity] */
  uint64_t *count;                /* device: groups listed (may exceed capacity) */
} qe_ready_out;

typedef struct qe_advance_opt {
  const uint8_t  *auto_leave;          /* [G] or NULL: Config.AutoLeave */
  const uint64_t *pending_conf_index;  /* [G], with auto_leave */
  uint32_t reserved[2];                /* must be 0 */
} qe_advance_opt;

int qe_ready_note(const qe_progress *p, const qe_ready_state *rs, const qe_ready_note_in *in,
                  void *stream);
size_t qe_ready_scratch_bytes(uint64_t num_groups);
int qe_ready(const qe_progress *p, const qe_follower *f, const qe_ready_state *rs,
             const qe_ready_in *in, const qe_ready_out *out, void *scratch, uint64_t *stats,
             void *stream);
/* f and opt may be NULL (no AutoLeave check). */
int qe_advance(const qe_progress *p, const qe_follower *f, const qe_ready_state *rs,
               const qe_ready_out *list, const qe_advance_opt *opt, uint8_t *result, void *stream);

/* qe_read_note / qe_read_states (additive in ABI 8): the answers to ReadIndex
 * requests as a dense device list -- the ReadStates of a Ready and the
 * MsgReadIndexResp messages, the part of a Ready that qe_ready (rule 6) leaves
 * to its `pending` row.  The queue of qe_progress (read_acks / read_head /
 * read_count / read_keys) holds a pending request's acks and key; what
 * readOnly.pendingReadIndex keeps besides (readIndexStatus.index and the
 * request's origin, raft/read_only.go:29-37) is resident in the request book,
 * so a host no longer keeps a map context -> (index, from) per group, copies
 * read_released / term_commit / term_commit_index [G] every step, or decides
 * responseToReadIndexReq (raft/raft.go:1737-1751) itself: it copies min(*count,
 * capacity) records.
 *
 * qe_read_book, two resident rows [G][cap], read-write, device; cap =
 * p->read_cap, or QE_READ_QUEUE when read_cap is 0.  The request with context c
 * of group g is at [g*cap + c % cap], the addressing of p->read_keys:
 *   req_index   readIndexStatus.index: the read index of the request
 *   req_from    req.From as a slot; >= num_slots = None (a local request)
 * An entry is valid while its context is pending and stays readable after its
 * release until a later request takes the slot.  The book needs no clearing
 * at a stepdown or in qe_become_leader: only contexts the queue names are read.
 *
 * qe_read_note: addRequest's bookkeeping half (read_only.go:56-63).  It takes
 * the rows a qe_read_index call wrote, result / ctx [G], and the caller's index
 * [G] and from [G] (NULL = every request is local: 0xFF is stored).  Where
 * result[g] == QE_RI_QUEUED it stores index[g] and from[g] at ctx[g] % cap;
 * every other result writes nothing (a QE_RI_DUPLICATE keeps the first
 * request's entry, as addRequest does).  `index` is the caller's row on
 * purpose: a postponed read re-added after term_commit is noted at that
 * round's term_commit_index, not at the index the re-adding qe_read_index
 * returns (see qe_read_index; raft.go:1813-1834).  Of p it reads num_groups and
 * read_cap.  QE_EINVAL: a NULL p / b / result / ctx / index or a NULL row of b;
 * a nonzero reserved3; read_acks with a read_cap above QE_READ_QUEUE and no
 * read_ovf (as wherever the queue's capacity is read); QE_ERANGE: read_cap
 * outside 0, QE_READ_QUEUE..QE_READ_CAP_MAX.  num_groups == 0 is QE_OK.
 *
 * qe_read_states.  Of p it reads num_groups (G), group_offset, num_slots (S),
 * read_cap, read_head, self_slot (NULL: no slot is the group's own) and
 * read_keys (NULL: keys not tracked).  Every row of `in` is optional:
 * read_released / term_commit / term_commit_index are the output rows of the
 * qe_progress_step just run, ri_result / ri_index / ri_key / ri_from the rows of
 * a qe_read_index call and its requests' origins.
 *  1. Ordering.  Records go by ascending group; within a group: the released
 *     requests in queue order (oldest first, as readOnly.advance returns them,
 *     read_only.go:85-112), then the TERM_COMMIT record, then the record of an
 *     immediate answer.
 *  2. Released requests.  k = read_released[g] requests were released; their
 *     contexts are read_head[g] - k + j (mod 2^32), j < k, with read_head read
 *     as it is after the step.  Contexts of a pending queue never cross 0
 *     (qe_read_index refuses with QE_RI_FULL), so this is exact.  Each yields
 *     ctx = c, index = req_index[g*cap + c % cap] and key = read_keys[g*cap +
 *     c % cap] when keys are tracked, else 0.
 *  3. Kind.  With f = req_from[g*cap + c % cap]: f >= num_slots, or f ==
 *     self_slot[g], gives QE_RS_STATE with to = 0xFF (req.From == None ||
 *     req.From == r.id: r.readStates gets ReadState{Index, RequestCtx});
 *     otherwise QE_RS_RESP with to = f (MsgReadIndexResp{To: req.From, Index,
 *     Entries: req.Entries}).
 *  4. TERM_COMMIT.  term_commit[g] != 0 gives one QE_RS_TERM_COMMIT record
 *     with index = term_commit_index[g], to = 0xFF, ctx = 0, key = 0: the host
 *     adds its postponed reads again (qe_read_index) and notes them at `index`.
 *  5. Immediate answers.  ri_result[g] == QE_RI_RESPOND (IsSingleton or
 *     lease-based, raft.go:1080-1084, :1838-1841) gives one record by rule 3
 *     with f = ri_from[g] (a NULL ri_from: None), index = ri_index[g], key =
 *     ri_key[g] (0 with a NULL ri_key) and ctx = 0.
 *  6. Capacity.  *count is the full number of records; nothing at or past
 *     min(*count, capacity) is touched in any output array (qe_outbox rule 3).
 *  7. State.  Nothing resident is written.
 *  8. Call order.  The call runs after the step whose rows it takes and
 *     before the next qe_read_index on the same state: a later request may
 *     take a released slot of the book (and of read_keys).
 *  9. stats (optional), over every record, those past capacity too:
 *     QE_STAT_GROUPS += groups with at least one record; QE_STAT_READ_STATE /
 *     _RESP / _TERM_COMMIT += records by kind; QE_STAT_CHECKSUM += h3 per
 *     record, h1 = mix64(group * 0x9E3779B97F4A7C15 ^ 0xE7037ED1A0B428DB ^ kind
 *     << 56 ^ to << 48 ^ ctx), h2 = mix64(h1 ^ index), h3 = mix64(h2 ^ key), as
 *     the record holds them (key 0 where it has none).
 * `count` and every array of qe_read_states_out are DEVICE pointers; `key` may
 * be NULL (not written).  scratch is qe_read_states_scratch_bytes(num_groups)
 * bytes of device memory, 8-B aligned (the chunk offsets and counts of
 * qe_collect).  Stream-ordered: three kernels (count, the scan of qe_collect,
 * fill), no host synchronisation.
 * QE_EINVAL: a NULL p / in / out / count / scratch (with num_groups > 0);
 * read_released with a NULL b, a NULL row of b, or a NULL read_head /
 * read_count; term_commit without term_commit_index; ri_result without
 * ri_index; capacity > 0 with a NULL group / kind / to / ctx / index; a nonzero
 * reserved field; num_slots outside 1..16; read_acks with a read_cap above
 * QE_READ_QUEUE and no read_ovf; scratch not 8-B aligned.  QE_ERANGE: a
 * read_cap out of range; more chunks than a launch holds (qe_ready's check).
 * Every argument check runs before the first HIP call.  num_groups == 0, or
 * every row of `in` NULL, is QE_OK with *count = 0. */
#define QE_RS_STATE 1        /* local ReadState{Index, RequestCtx} */
#define QE_RS_RESP 2         /* MsgReadIndexResp{To, Index, Entries = the request's} */
#define QE_RS_TERM_COMMIT 3  /* releasePendingReadIndexMessages fired: re-add the
                                postponed reads at `index` */
#define QE_STAT_READ_STATE QE_STAT_VOTE_WON             /* qe_read_states: records by kind */
#define QE_STAT_READ_RESP QE_STAT_VOTE_PENDING
#define QE_STAT_READ_TERM_COMMIT QE_STAT_COMMIT_ADVANCED

typedef struct qe_read_book {
  uint64_t *req_index;   /* [G][cap] rw: readIndexStatus.index of the request with context c,
                            at [g*cap + c % cap] (the addressing of qe_progress.read_keys) */
  uint8_t  *req_from;    /* [G][cap] rw: req.From as a slot; >= num_slots = None (local) */
} qe_read_book;

typedef struct qe_read_states_in {
  const uint8_t  *read_released;      /* [G] or NULL: qe_peer_msgs.read_released of the step just run */
  const uint8_t  *term_commit;        /* [G] or NULL */
  const uint64_t *term_commit_index;  /* [G], with term_commit */
  const uint8_t  *ri_result;          /* [G] or NULL: a qe_read_index call's result row */
  const uint64_t *ri_index;           /* [G], with ri_result */
  const uint8_t  *ri_from;            /* [G] or NULL (local), with ri_result */
  const uint64_t *ri_key;             /* [G] or NULL, with ri_result */
  uint32_t reserved[2];               /* must be 0 */
} qe_read_states_in;

typedef struct qe_read_states_out {
  uint64_t capacity;
  uint64_t *group;     /* [capacity] group_offset + g */
  uint8_t  *kind;      /* [capacity] QE_RS_* */
  uint8_t  *to;        /* [capacity] slot of a MsgReadIndexResp; 0xFF otherwise */
  uint32_t *ctx;       /* [capacity] context number; 0 for records that have none */
  uint64_t *index;     /* [capacity] ReadState.Index / m.Index / term_commit_index */
  uint64_t *key;       /* [capacity] or NULL: the request's key (read_keys / ri_key), else 0 */
  uint64_t *count;     /* device: the full number, may exceed capacity */
} qe_read_states_out;

int qe_read_note(const qe_progress *p, const qe_read_book *b, const uint8_t *result,
                 const uint32_t *ctx, const uint64_t *index, const uint8_t *from, void *stream);
size_t qe_read_states_scratch_bytes(uint64_t num_groups);
/* b may be NULL without read_released. */
int qe_read_states(const qe_progress *p, const qe_read_book *b, const qe_read_states_in *in,
                   const qe_read_states_out *out, void *scratch, uint64_t *stats, void *stream);

/* qe_requests (additive in ABI 8): a list of client requests handled as
 * raft.Step would on their receiver -- the one way into Step the calls above
 * leave to the host.  Propose, ReadIndex and TransferLeadership may be called
 * on any node, and a MsgReadIndexResp comes back to a follower; the engine has
 * the leader's arms (qe_propose, qe_read_index, QE_MSG_TRANSFER_LEADER of
 * qe_progress_step).  This call adds stepFollower's arms (raft/raft.go:
 * 1423-1432, :1445-1451, :1458-1470), stepCandidate's MsgProp drop (:1387-1389),
 * Step's term preamble for the two types that carry a term, and the routing of
 * the list into the leader-side rows, so a host keeps neither state nor lead
 * off the device and builds no G-sized row on the CPU.  It READS the list,
 * f->term, f->state and f->lead; of p it reads num_groups (G), group_offset,
 * num_slots (S), stride and self_slot (required) and nothing else.  It writes
 * nothing resident: only the rows of qe_requests_out, which the caller points
 * at the buffers it then passes on (rule 7), the dispositions and two dense
 * lists.
 *
 * The list is in arrival order; a record's position i is its rank.  `from` is
 * a slot in the receiver's numbering, or 0xFF = None: a local call without
 * From.  `term` is 0 for a local call and for a request forwarded without a
 * term.  `key` is the 64-bit request key qe_read_index / read_keys use as
 * RequestCtx.  The types continue the QE_IMSG_* numbering, so a transport has
 * one record format; qe_inbox itself still answers QE_ID_BAD for 17..19.
 *
 *  1. BAD.  A record gets QE_QD_BAD when its group is outside [group_offset,
 *     group_offset + G); its type is none of QE_QMSG_*; its from is neither
 *     < S nor 0xFF; it is a PROP with num_entries == 0 (stepLeader panics on
 *     an empty MsgProp, raft.go:1020-1022); it is a PROP or READ_INDEX with
 *     term != 0 (send never attaches one, :410-416); or it is a
 *     TRANSFER_LEADER with from == 0xFF (m.From is the transferee).  It takes
 *     no further part and is never deferred.
 *  2. Preamble.  A record with term == 0 is local and passes (:850-851).
 *     Otherwise, with r.Term = f->term[g]:
 *     a. term < r.Term: QE_QD_DROP_LOWER_TERM (:883-919: none of these types
 *        is answered);
 *     b. term > r.Term: QE_QD_STEPDOWN.  The vote rows at [g] get v_type =
 *        QE_VMSG_VOTE_RESP with from, term, index and log_term 0 and flags
 *        QE_VMF_REJECT (qe_inbox rule 6c: becomeFollower(m.Term, None) runs in
 *        qe_vote_step).  What stepFollower does next is decided at once: a
 *        READ_INDEX_RESP also yields its READ_STATE output record (rule 5); a
 *        TRANSFER_LEADER yields nothing, because lead is None after the
 *        stepdown (:1446-1449).
 *  3. By role (f->state[g]), for a record that passed rule 2:
 *     a. QE_STATE_LEADER.  PROP: QE_QD_ROUTED into the proposal rows at [g]:
 *        p_num_entries, p_payload, p_cc_count and all max_cc conf-change rows
 *        p_cc_pos / p_cc_leave / p_cc_size at [k*cc_stride+g] (zeros included).
 *        READ_INDEX: ROUTED into ri_request[g] = 1, ri_key[g] = key, ri_from[g]
 *        = from.  TRANSFER_LEADER: ROUTED into r_type[from*stride+g] =
 *        QE_MSG_TRANSFER_LEADER.  READ_INDEX_RESP: QE_QD_NO_ARM (stepLeader has
 *        no arm for it).
 *     b. QE_STATE_CANDIDATE / _PRE_CANDIDATE.  PROP: QE_QD_PROP_DROPPED
 *        (ErrProposalDropped, :1387-1389); every other type: QE_QD_NO_ARM.
 *     c. Any other state is a follower, with lead = f->lead[g] (>= S = None).
 *        PROP: no lead, or QE_REQ_NO_FORWARD (Config.
 *        DisableProposalForwarding), gives QE_QD_PROP_DROPPED (:1424-1430);
 *        otherwise QE_QD_FORWARDED (:1431-1432).  READ_INDEX: no lead gives
 *        QE_QD_NO_LEADER (a silent drop, :1459-1462), otherwise FORWARDED.
 *        TRANSFER_LEADER: no lead gives NO_LEADER (:1446-1449); with a lead
 *        and term == 0 FORWARDED; with a lead and a nonzero term
 *        QE_QD_REF_PANIC: the reference's send panics on a set term
 *        (:407-409); the record is not forwarded and is counted in
 *        QE_STAT_INVARIANT_VIOLATIONS.  READ_INDEX_RESP: QE_QD_READ_STATE
 *        (:1465-1470; a record has exactly one key, so the len(Entries) != 1
 *        check has no counterpart).
 *  4. Order within a group.  The records of a group are handled in list order
 *     until the first ROUTED or STEPDOWN record.  That record closes the
 *     group: every later record of the group that is not BAD gets
 *     QE_QD_DEFERRED.  So a group gets at most one row-writing record per pass
 *     and the relative order of, say, a transfer and a proposal is kept
 *     exactly; the records before the closer write no state, so any number of
 *     them is handled in one pass.
 *  5. Output list: dense, ascending in list position, one record for each
 *     FORWARDED, READ_STATE (a STEPDOWN READ_INDEX_RESP's included) and
 *     PROP_DROPPED record.  group; kind = QE_QO_FWD / _READ_STATE /
 *     _PROP_DROPPED; type = the input type; to = the lead slot for FWD, else
 *     0xFF; from = for FWD the record's from where it is a slot, else
 *     self_slot[g] (send fills From only when it is None, :387-389; a forwarded
 *     From is kept), else 0xFF; term = f->term[g] for a forwarded
 *     TRANSFER_LEADER, else 0 (PROP and READ_INDEX go without a term); index =
 *     the record's index for READ_STATE, else 0; key; src = the list position.
 *     *count is the full number of records; nothing at or past min(*count,
 *     capacity) is touched in any output array (qe_outbox rule 3).  A FWD
 *     TRANSFER_LEADER record has type 10 and carries its term: the receiving
 *     host may hand it to qe_inbox or to this call as it is.
 *  6. Rows.  p_num_entries, ri_request, v_type [G] and r_type (columns < G of
 *     each of the S slot rows; the pad columns are not touched) are COMPLETE: 0
 *     where nothing was routed.  Every other row is written only where its
 *     complete row is non-zero.  p_src / ri_src / v_src [G] and r_src
 *     [S][stride] (each optional) get the list position of the routed record.
 *     disposition[i] = QE_QD_* of every record.  deferred[0 .. *deferred_count)
 *     = the positions of the DEFERRED records, ascending; the next pass's list
 *     is those records followed by what arrived since.
 *  7. Consequences.  A request pass is a pass of its own: its rows are not
 *     merged with qe_inbox's rows of the same round.  In the order a host
 *     calls the steps on them the rows feed qe_propose, qe_read_index
 *     (ri_request, ri_key), qe_read_note (from = ri_from), qe_progress_step,
 *     qe_vote_step and qe_read_states (ri_*).  Because of rule 4 no two of
 *     these touch the same group.
 *  8. stats (optional): QE_STAT_GROUPS += groups with a ROUTED record;
 *     QE_STAT_REQ_* += records by disposition, BAD and REF_PANIC also into
 *     QE_STAT_INVARIANT_VIOLATIONS; QE_STAT_CHECKSUM += mix64(mix64(group *
 *     0x9E3779B97F4A7C15 ^ 0xA24BAED4963EE407 ^ disposition << 56 ^ type << 48 ^
 *     from << 40) ^ i) per list record.
 * Every array is a DEVICE pointer; scratch is qe_requests_scratch_bytes(G,
 * num_records) bytes of device memory, 8-B aligned: 4 * G + 2 * n bytes plus 2 *
 * qe_collect_scratch_bytes(n) -- one word per group (qe_inbox: 3 + S), two flag
 * bytes per record and qe_collect's part for each of the two lists.
 * Stream-ordered, no host synchronisation: an init pass over the groups, two
 * passes over the records, and per list qe_collect's count and scan and a fill
 * of the record-list layer.  Positions are keys of 32-bit atomicMin, which is
 * order-free: the outputs are bit-exact from run to run.
 * QE_ERANGE: num_records > 0xFFFFFFF0.
 * QE_EINVAL: a NULL p / f / in / out; f->term, f->state or f->lead NULL;
 * p->self_slot NULL; num_slots outside 1..16 or a nonzero reserved field of p;
 * in->reserved nonzero; a bit of in->flags other than QE_REQ_NO_FORWARD; stride
 * < num_groups; max_cc > QE_PROP_MAX_CC; max_cc > 0 with cc_stride < num_groups
 * or a NULL p_cc_count / p_cc_pos / p_cc_leave / p_cc_size, or with in->cc_count
 * and a NULL in->cc_pos / cc_leave / cc_size; num_records > 0 with a NULL group /
 * type / from / term / index / key (num_entries, payload and cc_count may be
 * NULL: zeros, none); a NULL p_num_entries / ri_request / ri_key / ri_from /
 * v_type / v_from / v_term / v_index / v_log_term / r_type / disposition /
 * deferred / deferred_count / count; capacity > 0 with a NULL array of the
 * output list; scratch NULL (with num_groups > 0) or not 8-B aligned.  Every
 * argument check runs before the first HIP call.  num_records == 0 is QE_OK
 * with complete rows and both counts 0; num_groups == 0 is QE_OK with both
 * counts 0 and nothing else written. */
#define QE_QMSG_TRANSFER_LEADER 10    /* MsgTransferLeader (= QE_IMSG_TRANSFER_LEADER) */
#define QE_QMSG_PROP 17               /* MsgProp          */
#define QE_QMSG_READ_INDEX 18         /* MsgReadIndex     */
#define QE_QMSG_READ_INDEX_RESP 19    /* MsgReadIndexResp */
#define QE_QD_ROUTED 1            /* in this pass's rows (= QE_ID_ROUTED)      */
#define QE_QD_STEPDOWN 2          /* a higher term, as a vote row              */
#define QE_QD_DEFERRED 3          /* waits for the next pass                   */
#define QE_QD_DROP_LOWER_TERM 4
#define QE_QD_NO_ARM 5            /* the receiver's step function ignores it   */
#define QE_QD_FORWARDED 6         /* to the lead: a QE_QO_FWD record           */
#define QE_QD_READ_STATE 7        /* a QE_QO_READ_STATE record                 */
#define QE_QD_PROP_DROPPED 8      /* ErrProposalDropped: a QE_QO_PROP_DROPPED record */
#define QE_QD_NO_LEADER 9         /* a follower without a lead drops it silently */
#define QE_QD_REF_PANIC 10        /* the reference would panic; nothing is sent */
#define QE_QD_BAD 255
#define QE_QO_FWD 1               /* the request, addressed to the lead        */
#define QE_QO_READ_STATE 2        /* ReadState{Index: index, RequestCtx: key}  */
#define QE_QO_PROP_DROPPED 3      /* ErrProposalDropped for the caller         */
#define QE_REQ_NO_FORWARD 1u      /* Config.DisableProposalForwarding, batch-wide */
#define QE_STAT_REQ_BAD QE_STAT_COMMIT_INF              /* qe_requests: records by disposition */
#define QE_STAT_REQ_NO_ARM QE_STAT_COMMIT_SUM
#define QE_STAT_REQ_NO_LEADER QE_STAT_COMMIT_ZERO
#define QE_STAT_REQ_ROUTED QE_STAT_VOTE_WON
#define QE_STAT_REQ_LOWER_TERM QE_STAT_VOTE_LOST
#define QE_STAT_REQ_DEFERRED QE_STAT_VOTE_PENDING
#define QE_STAT_REQ_FORWARDED QE_STAT_GRANTED
#define QE_STAT_REQ_PROP_DROPPED QE_STAT_REJECTED
#define QE_STAT_REQ_READ_STATE QE_STAT_COMMIT_ADVANCED
#define QE_STAT_REQ_REF_PANIC QE_STAT_READ_RELEASED
#define QE_STAT_REQ_STEPDOWN QE_STAT_STEPDOWNS

typedef struct qe_requests_in {
  uint64_t num_records;         /* n <= 0xFFFFFFF0 */
  uint32_t max_cc;              /* conf-change rows per record, <= QE_PROP_MAX_CC */
  uint32_t flags;               /* QE_REQ_NO_FORWARD or 0 */
  const uint64_t *group;        /* [n] the RECEIVER's global group id */
  const uint8_t  *type, *from;  /* [n] QE_QMSG_*; a slot in the receiver's numbering or 0xFF */
  const uint64_t *term;         /* [n] 0 = local, or forwarded without a term */
  const uint64_t *index;        /* [n] m.Index of a READ_INDEX_RESP */
  const uint64_t *key;          /* [n] the request key of a READ_INDEX / READ_INDEX_RESP */
  const uint32_t *num_entries;  /* [n] or NULL (zeros): len(m.Entries) of a PROP */
  const uint64_t *payload;      /* [n] or NULL (zeros): qe_proposals.payload */
  const uint8_t  *cc_count;     /* [n] or NULL (none): qe_proposals.cc_count */
  const uint32_t *cc_pos;       /* [max_cc][n] */
  const uint8_t  *cc_leave;     /* [max_cc][n] */
  const uint32_t *cc_size;      /* [max_cc][n] */
  uint64_t reserved;            /* must be 0 */
} qe_requests_in;

typedef struct qe_requests_out {
  uint32_t *p_num_entries;      /* [G] qe_proposals; complete */
  uint64_t *p_payload;          /* [G] or NULL */
  uint8_t  *p_cc_count;         /* [G]; may be NULL with max_cc 0 */
  uint32_t *p_cc_pos;           /* [max_cc][cc_stride] */
  uint8_t  *p_cc_leave;         /* [max_cc][cc_stride] */
  uint32_t *p_cc_size;          /* [max_cc][cc_stride] */
  uint64_t cc_stride;           /* >= num_groups (read with max_cc > 0) */
  uint8_t  *ri_request;         /* [G] qe_read_index's request row; complete */
  uint64_t *ri_key;             /* [G] qe_read_index's key row */
  uint8_t  *ri_from;            /* [G] qe_read_note's / qe_read_states' from row */
  uint8_t  *v_type, *v_from;    /* [G] qe_vote_msgs; v_type complete */
  uint64_t *v_term, *v_index, *v_log_term;
  uint8_t  *v_flags;            /* [G] or NULL */
  uint8_t  *r_type;             /* [S][stride] qe_peer_msgs.type; complete in the columns < G */
  uint32_t *p_src, *ri_src, *v_src;  /* [G], each or NULL */
  uint32_t *r_src;              /* [S][stride] or NULL */
  uint8_t  *disposition;        /* [n] QE_QD_* */
  uint32_t *deferred;           /* [n] positions of the DEFERRED records, ascending */
  uint64_t *deferred_count;     /* device */
  uint64_t capacity;            /* of the output list */
  uint64_t *group;              /* [capacity] */
  uint8_t  *kind, *type;        /* [capacity] QE_QO_*, QE_QMSG_* */
  uint8_t  *to, *from;          /* [capacity] slots, 0xFF = none */
  uint64_t *term, *index, *key; /* [capacity] */
  uint32_t *src;                /* [capacity] the record's list position */
  uint64_t *count;              /* device: the full number, may exceed capacity */
} qe_requests_out;

size_t qe_requests_scratch_bytes(uint64_t num_groups, uint64_t num_records);
int qe_requests(const qe_progress *p, const qe_follower *f, const qe_requests_in *in,
                const qe_requests_out *out, void *scratch, uint64_t *stats, void *stream);

/* qe_apply_conf (additive in ABI 8): committed conf-change entries applied as a
 * device list, on every role -- RawNode.ApplyConfChange -> raft.applyConfChange
 * -> switchToConfig (raft/rawnode.go:104-107, raft/raft.go:1623-1700).  A host
 * lists the ConfChangeV2 entries a Ready handed it to apply (a V1 ConfChange as
 * its AsV2 form: QE_AC_AUTO with one change) and gets back, per record, what
 * happened and the ConfState ApplyConfChange returns.  It builds no [G] row
 * (op, count, last_index, switched) and reads none (state, the masks).
 *
 * The list: n records, n = min(*in->count, capacity) when in->count (DEVICE) is
 * given, else min(in->n, capacity), as qe_advance reads its list.  Record i:
 *   group[i]          absolute; g = group[i] - p->group_offset
 *   transition[i]     QE_AC_AUTO, QE_AC_JOINT_IMPLICIT, QE_AC_JOINT_EXPLICIT
 *                     (ConfChangeTransition, raft/raftpb/raft.pb.go)
 *   num_changes[i]    its ConfChangeSingle entries, <= max_changes (C)
 *   type[k*capacity+i], node_id[k*capacity+i]   change k (QE_CC_ADD_NODE ...;
 *                     node 0 = ignored, as qe_confchange)
 *   slot[k*capacity+i]   optional row: the slot a change that creates a
 *                     Progress must take; QE_AC_ANY_SLOT (0xFF), or a NULL
 *                     row, is qe_confchange's rule, the lowest untracked slot.
 *                     A named slot that is tracked or >= num_slots makes the
 *                     change fail with QE_CC_ERR_NO_SLOT.  A host that keeps
 *                     slot = node (the layout qe_outbox / qe_inbox / qe_replies
 *                     route by) names the slot of every added id.
 * The records are in non-decreasing group order; the records of one group are
 * a run of neighbours, applied in list order.
 *
 * Per record, result[i] (QE_AC_*), cc_result[i] (QE_CC_*), sw_result[i]
 * (QE_SW_*):
 *  1. Decode (raft/raftpb/confchange.go:71-107).  num_changes == 0 and
 *     transition == QE_AC_AUTO: LeaveJoint.  Else transition != QE_AC_AUTO or
 *     num_changes > 1: EnterJoint with autoLeave = transition !=
 *     QE_AC_JOINT_EXPLICIT.  Else Simple.
 *  2. Changer (raft/confchange/confchange.go:49-274) with LastIndex =
 *     p->last_index[g], on the rows of c, exactly as qe_confchange runs it: on
 *     success only the words of c that changed are written (a created slot's
 *     id, 0 for a slot that lost its Progress), the created slots' Progress in
 *     p is initialised (Match 0, Next = last_index, StateProbe, RecentActive,
 *     no pending snapshot) and cc_result = QE_CC_OK.  p->inc_mask / out_mask /
 *     tracked are switchToConfig's view of the new configuration.  ALIASING:
 *     each of the three is either the very pointer of c's inc_mask / out_mask /
 *     tracked (one row serves both; the usual set-up) or memory that overlaps
 *     no row of c, and is then written too (all three words of the group, on
 *     every applied record).  No other row of c, p, f, in, out or scratch may
 *     overlap another.
 *  3. Role.  f->state[g] != QE_STATE_LEADER: switchToConfig returns at :1678,
 *     result = QE_AC_APPLIED, sw_result = QE_SW_NONE.  A leader: result =
 *     QE_AC_LEADER and sw_result is the QE_SW_* byte (QE_SW_TRANSFER_ABORTED
 *     included) of switchToConfig's leader half, which qe_switch_config's
 *     kernel runs after the list on the groups this call marked in scratch;
 *     p->self_slot tells it whether the leader still has a Progress
 *     (QE_SW_REMOVED).  sw->result / sent / snap ([G], device) are filled for
 *     every group as qe_switch_config fills them (0 for a group not switched),
 *     so qe_outbox consumes sent / snap unchanged; sw->switched is not read.
 *     State, stores and result bytes of the leader half are those of
 *     qe_confchange followed by qe_switch_config on the same state.
 *  4. Several records of one group.  A group that does not lead applies them
 *     all, in list order, each on the configuration its predecessor left.  A
 *     leader applies the first; each later one is QE_AC_DEFERRED and nothing is
 *     done for it (the sends of the first are harvested with qe_outbox first,
 *     then the host lists the deferred records again).
 *  5. Refusals, result >= QE_AC_REFUSED: nothing of the group is written by
 *     the record.
 *       QE_AC_BAD_GROUP      g outside [0, num_groups)
 *       QE_AC_BAD_ORDER      group[i] < group[i-1].  (A list out of order may
 *                            name a group in two runs; what those runs leave
 *                            of it is unspecified, memory stays in bounds.)
 *       QE_AC_BAD_CHANGE     transition > 2 or num_changes > max_changes
 *       QE_AC_CHANGER_ERROR  the Changer refused: the reference's panic
 *                            (:1637-1640); cc_result = the QE_CC_ERR_*
 *       QE_AC_SKIPPED        an earlier record of the run was refused
 *     A refusal ends its run: every later record of the group is SKIPPED.
 *  6. The ConfState (ProgressTracker.ConfState, tracker.go:146-154) after the
 *     record, in slot form: inc (Voters), out (VotersOutgoing), learner,
 *     learners_next, tracked (mask-typed), auto_leave, new_progress (the slots
 *     whose Progress this record created), and with ids ([S][capacity]) the id
 *     of every tracked slot, 0 elsewhere.  A DEFERRED, SKIPPED, BAD_CHANGE or
 *     CHANGER_ERROR record shows the configuration as it stands; a record of a
 *     BAD_GROUP or BAD_ORDER run shows zeros.  Nothing at or past n is touched
 *     in any output array.
 * scratch: qe_apply_conf_scratch_bytes(num_groups) bytes of device memory,
 * 16-B aligned, owned by the call: it clears what it needs (the `switched`
 * row, G bytes) itself, so calls follow each other on one stream with no host
 * work between them.  Stream-ordered, four kernels (clear, the list, the
 * switch kernel over the batch, the gather of sw_result), no host
 * synchronisation.  Of p the list kernel reads num_groups, group_offset,
 * num_slots, stride, last_index and writes match / next / pending_snapshot /
 * peer of the created slots; the switch kernel reads and writes what
 * qe_switch_config does.
 * QE_EINVAL: a NULL p / f / c / in / out / scratch; whatever qe_switch_config
 * refuses in p (its QE_ERANGE cases stay QE_ERANGE); a NULL f->state; a NULL
 * p->inc_mask / out_mask / tracked / self_slot; c->num_groups or num_slots
 * other than p's, a nonzero c->reserved, a NULL row of c; a nonzero
 * in->reserved, max_changes > 255; capacity > 0 with a NULL group / transition
 * / num_changes, or with max_changes > 0 and a NULL type / node_id; capacity >
 * 0 with a NULL result / cc_result / sw_result / inc / out / learner /
 * learners_next / tracked / new_progress / auto_leave (ids may be NULL); sw
 * with a NULL result or a non-NULL bytes_requested; scratch not 16-B aligned.
 * Every argument check runs before the first HIP call.  capacity == 0 or
 * num_groups == 0 is QE_OK: nothing is written. */
#define QE_AC_AUTO 0              /* ConfChangeTransitionAuto */
#define QE_AC_JOINT_IMPLICIT 1    /* ConfChangeTransitionJointImplicit */
#define QE_AC_JOINT_EXPLICIT 2    /* ConfChangeTransitionJointExplicit */
#define QE_AC_ANY_SLOT 0xFFu      /* slot: the lowest untracked one */
#define QE_AC_APPLIED 1           /* applied; the group does not lead */
#define QE_AC_LEADER 2            /* applied by a leader: sw_result holds the QE_SW_* */
#define QE_AC_DEFERRED 3          /* a leader's later record: list it again */
#define QE_AC_REFUSED 16          /* results >= this: nothing of the group written */
#define QE_AC_BAD_GROUP 16
#define QE_AC_BAD_ORDER 17
#define QE_AC_BAD_CHANGE 18
#define QE_AC_CHANGER_ERROR 19
#define QE_AC_SKIPPED 20

typedef struct qe_apply_conf_in {
  uint64_t capacity;            /* records the arrays of in and out hold */
  uint64_t n;                   /* records listed (read when count is NULL) */
  const uint64_t *count;        /* device, or NULL: records listed */
  uint32_t max_changes;         /* C, changes per record at most, <= 255 */
  uint32_t reserved;            /* must be 0 */
  const uint64_t *group;        /* [capacity] */
  const uint8_t  *transition;   /* [capacity] QE_AC_AUTO ... */
  const uint8_t  *num_changes;  /* [capacity] */
  const uint8_t  *type;         /* [C][capacity] QE_CC_ADD_NODE ... */
  const uint64_t *node_id;      /* [C][capacity] */
  const uint8_t  *slot;         /* [C][capacity] or NULL */
} qe_apply_conf_in;

typedef struct qe_apply_conf_out {
  uint8_t *result;              /* [capacity] QE_AC_* */
  uint8_t *cc_result;           /* [capacity] QE_CC_* */
  uint8_t *sw_result;           /* [capacity] QE_SW_* */
  void *inc, *out;              /* [capacity] mask-typed: Voters, VotersOutgoing */
  void *learner, *learners_next; /* [capacity] mask-typed */
  void *tracked;                /* [capacity] mask-typed */
  void *new_progress;           /* [capacity] mask-typed */
  uint8_t *auto_leave;          /* [capacity] */
  uint64_t *ids;                /* [S][capacity] or NULL */
} qe_apply_conf_out;

size_t qe_apply_conf_scratch_bytes(uint64_t num_groups);
/* sw may be NULL (the [G] rows of the leader half are not wanted). */
int qe_apply_conf(const qe_progress *p, const qe_follower *f, const qe_conf *c,
                  const qe_apply_conf_in *in, const qe_apply_conf_out *out,
                  const qe_switch *sw, void *scratch, void *stream);

/* ---- statistics -------------------------------------------------------- */

/* out[QE_STATS_COUNTERS] (device) = sum over shards of stats (device). */
int qe_stats_reduce(const uint64_t *stats, uint64_t *out, void *stream);

/* ---- multi-GPU aggregation (RCCL over xGMI) ---------------------------- */

/* Groups shard across GPUs with no data-path exchange; the one collective is
 * the sum of the statistics vector (the batch form of etcd's per-member
 * Prometheus counters, server/etcdserver/metrics.go:29-85).  Setup: rank 0
 * calls qe_comm_unique_id, the host sends those qe_comm_id_bytes() bytes to
 * every rank over its own transport, every rank calls qe_comm_init with its
 * rank and device.  One communicator per process (one process per GPU). */
size_t qe_comm_id_bytes(void);                 /* size of the id (128) */
int qe_comm_unique_id(void *id);               /* rank 0: new id (host) */
int qe_comm_init(void **comm, uint32_t nranks, uint32_t rank, const void *id,
                 int device);
/* qe_comm_init with a bound (ABI 6): the communicator is created
 * non-blocking and polled; when the other ranks have not joined after
 * timeout_ms (e.g. one of them failed before calling init) it is aborted and
 * QE_ECOMM returned, so no rank waits forever.  timeout_ms == 0: blocking,
 * as qe_comm_init.  Hosts then agree over their own transport on the path
 * every rank takes (bench.py Dist._select_stats_path). */
int qe_comm_init_timeout(void **comm, uint32_t nranks, uint32_t rank, const void *id,
                         int device, uint32_t timeout_ms);
/* ncclCommFinalize (polled, at most 30 s, on a non-blocking communicator;
 * aborted when it does not complete: QE_ECOMM) then ncclCommDestroy. */
int qe_comm_destroy(void *comm);
/* ncclCommAbort (ABI 6): frees the communicator without waiting for its
 * outstanding collectives -- the way out when a peer failed mid-run. */
int qe_comm_abort(void *comm);

/* stats[0..n) (DEVICE, n <= QE_STATS_WORDS; normally the QE_STATS_COUNTERS
 * words qe_stats_reduce produced) = elementwise sum over all ranks of comm,
 * in place, asynchronously on `stream`: ncclAllReduce(ncclUint64, ncclSum).
 * uint64 addition wraps like the counters themselves.  On a non-blocking
 * communicator the enqueue is awaited (sleeping polls, at most 30 s; then
 * QE_ECOMM).  The collective completes only when every rank enqueued it: a
 * host should run it on a stream of its own, agree with its peers over its
 * own transport that every rank enqueued it, and bound its wait for the
 * completion (qe_comm_abort on failure) -- bench.py Dist.sum_stats. */
int qe_allreduce_stats(uint64_t *stats, uint32_t n, void *comm, void *stream);

/* ---- synthetic inputs (counter-based, bit-identical to oracle/) -------- */

typedef struct qe_gen_params {
  uint64_t seed;
  uint64_t group_offset;     /* global id of group 0                         */
  uint32_t dist;             /* 0 clustered, 1 uniform (Int63), 2 small ties */
  uint32_t p_absent_q16;     /* P(slot has no acked index) * 65536           */
  uint32_t p_voted_q16;      /* P(slot voted) * 65536                        */
  uint32_t p_granted_q16;    /* P(granted | voted) * 65536                   */
  uint32_t n_inc;            /* joint: incoming voters (0 = all S slots)     */
  uint32_t n_out;            /* joint: outgoing voters (0 = non-joint)       */
  uint32_t mask_mode;        /* 0 structured + rotated, 1 arbitrary random,
                                2 shape-bucketed (voters in low slots, overlap
                                constant per 2^20 consecutive groups)        */
  uint32_t reserved;
} qe_gen_params;

/* Fill a qe_groups batch (the pointers inside `g` are written through; the
 * const qualifiers of qe_groups are cast away).  Masks pointers that are
 * NULL in `g` are skipped. */
int qe_gen_groups(const qe_groups *g, const qe_gen_params *p, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ETCD_QUORUM_H */
