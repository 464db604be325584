"""ctypes binding of the C ABI in include/etcd_quorum.h (libetcd_quorum.so).

This is the same surface a cgo binding would use.  The
library is the product: if it is missing this module raises at import time
-- there is no CPU fallback.
"""
import ctypes as C
import os

# torch must be imported BEFORE the library is dlopen'ed: torch ships its own
# libamdhip64.so.7 and device memory / streams come from torch, so the
# library's DT_NEEDED libamdhip64.so.7 has to bind to that same runtime
# instance (two HIP runtimes in one process do not see each other's devices).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QE_LIB", os.path.join(_HERE, "lib", "libetcd_quorum.so"))

QE_ABI_VERSION = 8
QE_OK = 0
QE_EINVAL = -22
QE_ERANGE = -34
QE_EHIP = -1000
QE_ECOMM = -1001
QE_INDEX_INF = (1 << 64) - 1
QE_MAX_SLOTS = 16
QE_VOTE_PENDING, QE_VOTE_LOST, QE_VOTE_WON = 1, 2, 3
QE_STATE_FOLLOWER, QE_STATE_CANDIDATE, QE_STATE_LEADER, QE_STATE_PRE_CANDIDATE = 0, 1, 2, 3
QE_ELEC_PREVOTE, QE_ELEC_CHECK_QUORUM = 1, 2
QE_STATS_COUNTERS = 16
QE_STATS_SHARDS = 64
QE_STATS_WORDS = QE_STATS_COUNTERS * QE_STATS_SHARDS

STAT_NAMES = [
    "groups", "commit_inf", "commit_sum", "commit_zero", "vote_won", "vote_lost",
    "vote_pending", "granted", "rejected", "commit_advanced", "read_released", "elections",
    "leaders", "stepdowns", "invariant_violations", "checksum",
]

u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p


class QeGroups(C.Structure):
    _fields_ = [
        ("num_groups", u64), ("group_offset", u64), ("num_slots", u32), ("reserved", u32),
        ("stride", u64), ("match", vp), ("inc_mask", vp), ("out_mask", vp),
        ("learner_mask", vp), ("voted", vp), ("granted", vp),
    ]


class QeOutputs(C.Structure):
    _fields_ = [("commit", vp), ("vote", vp), ("granted_count", vp), ("rejected_count", vp),
                ("stats", vp)]


class QeReplState(C.Structure):
    _fields_ = [
        ("num_groups", u64), ("group_offset", u64), ("num_slots", u32), ("reserved", u32),
        ("stride", u64), ("match", vp), ("next", vp), ("committed", vp), ("term_start", vp),
        ("last_index", vp), ("inc_mask", vp), ("out_mask", vp),
    ]


class QeReplMsgs(C.Structure):
    _fields_ = [("resp_index", vp), ("resp_mask", vp), ("read_acks", vp), ("read_ok", vp),
                ("commit_advanced", vp)]


class QeElectionState(C.Structure):
    _fields_ = [
        ("num_groups", u64), ("group_offset", u64), ("num_slots", u32), ("reserved", u32),
        ("term", vp), ("state", vp), ("voted", vp), ("granted", vp), ("self_slot", vp),
        ("inc_mask", vp), ("out_mask", vp), ("learner_mask", vp),
    ]


class QeElectionParams(C.Structure):
    _fields_ = [("seed", u64), ("step0", u64), ("steps", u32), ("p_drop_q16", u32),
                ("p_grant_q16", u32), ("flags", u32), ("p_active_q16", u32), ("reserved", u32),
                ("script_resp", vp), ("script_grant", vp), ("script_hup", vp),
                ("script_stride", u64)]


class QeGenParams(C.Structure):
    _fields_ = [
        ("seed", u64), ("group_offset", u64), ("dist", u32), ("p_absent_q16", u32),
        ("p_voted_q16", u32), ("p_granted_q16", u32), ("n_inc", u32), ("n_out", u32),
        ("mask_mode", u32), ("reserved", u32),
    ]


class QeConfStateCSR(C.Structure):
    _fields_ = [("num_groups", u64), ("voters", vp), ("voters_off", vp),
                ("voters_outgoing", vp), ("outgoing_off", vp), ("learners", vp),
                ("learners_off", vp), ("learners_next", vp), ("learners_next_off", vp),
                ("auto_leave", vp), ("perm", vp)]


class QeProgress(C.Structure):
    _fields_ = [
        ("num_groups", u64), ("group_offset", u64), ("num_slots", u32), ("inflight_cap", u32),
        ("stride", u64), ("match", vp), ("next", vp), ("pending_snapshot", vp), ("peer", vp),
        ("infl_lo", vp), ("infl_hi", vp), ("committed", vp),
        ("term_start", vp), ("first_index", vp), ("last_index", vp), ("log_runs", u32),
        ("reserved", u32), ("run_first", vp), ("run_term", vp), ("run_count", vp),
        ("inc_mask", vp), ("out_mask", vp),
        ("tracked", vp), ("self_slot", vp), ("lead_transferee", vp), ("snap_index", vp),
        ("max_ents", u32), ("reserved2", u32),
        ("read_acks", vp), ("read_head", vp), ("read_count", vp),  # ABI 5
        ("read_cap", u32), ("reserved3", u32), ("read_ovf", vp), ("read_keys", vp),  # ABI 7
        ("infl16", vp),  # ABI 8: the 16-bit Inflights form
    ]


class QePeerMsgs(C.Structure):
    _fields_ = [("type", vp), ("index", vp), ("reject_hint", vp), ("log_term", vp),
                ("sent", vp), ("bcast", vp), ("snap", vp), ("timeout_now", vp),
                ("msg_count", vp), ("msg_index", vp), ("bytes_requested", vp),
                ("read_ctx", vp), ("read_released", vp), ("term_commit", vp),  # ABI 5
                ("term_commit_index", vp)]


class QeProposals(C.Structure):  # ABI 6
    _fields_ = [("num_entries", vp), ("payload", vp), ("max_cc", u32), ("flags", u32),
                ("cc_stride", u64), ("cc_count", vp), ("cc_pos", vp), ("cc_leave", vp),
                ("cc_size", vp), ("applied", vp), ("pending_conf_index", vp),
                ("uncommitted_size", vp), ("max_uncommitted", u64), ("result", vp),
                ("cc_refused", vp), ("sent", vp), ("snap", vp), ("bytes_requested", vp)]


class QeSwitch(C.Structure):  # ABI 7
    _fields_ = [("switched", vp), ("result", vp), ("sent", vp), ("snap", vp),
                ("bytes_requested", vp)]


class QeLeader(C.Structure):  # ABI 7
    _fields_ = [("elected", vp), ("term", vp), ("flags", u32), ("reserved", u32),
                ("pending_conf_index", vp), ("uncommitted_size", vp), ("result", vp),
                ("sent", vp), ("snap", vp)]


class QeTimers(C.Structure):  # qe_tick
    _fields_ = [("state", vp), ("timer", vp), ("randomized_timeout", vp), ("no_campaign", vp),
                ("events", vp), ("election_timeout", u32), ("heartbeat_timeout", u32),
                ("flags", u32), ("ticks", u32), ("seed", u64), ("tick_no", u64)]


class QeTickOut(C.Structure):  # qe_tick
    _fields_ = [("action", vp), ("hb_commit", vp), ("hb_ctx", vp), ("hb_sent", vp),
                ("quorum_active", vp)]


QE_TICK_CHECK_QUORUM = 1
QE_TEV_HEARD, QE_TEV_RESET = 1, 2
QE_TICK_HUP, QE_TICK_BEAT, QE_TICK_CHECKED_QUORUM, QE_TICK_STEPDOWN = 1, 2, 4, 8
QE_TICK_TRANSFER_ABORTED = 16

# qe_follower_step
QE_MAX_MSG_RUNS = 4
QE_FOLLOW_CHECK_QUORUM, QE_FOLLOW_PREVOTE = 1, 2
QE_LMSG_NONE, QE_LMSG_APP, QE_LMSG_HEARTBEAT = 0, 1, 2
QE_FR_NONE, QE_FR_IGNORED, QE_FR_LOWER_TERM_RESP, QE_FR_HEARTBEAT_RESP = 0, 1, 2, 3
QE_FR_APP_ACCEPT, QE_FR_APP_REJECT, QE_FR_APP_STALE = 4, 5, 6
QE_FR_REFUSED = 16  # results >= this: nothing of the group changed
QE_FR_BAD_MSG, QE_FR_COMMIT_PAST_LOG, QE_FR_CONFLICT_COMMITTED, QE_FR_RUNS_FULL = 16, 17, 18, 19
QE_FR_APP_GAP = 20
QE_STAT_FOLLOW_APPENDED = 2  # = QE_STAT_COMMIT_SUM


class QeFollower(C.Structure):
    _fields_ = [("term", vp), ("state", vp), ("lead", vp), ("vote", vp), ("flags", u32),
                ("reserved", u32)]


class QeLeaderMsgs(C.Structure):
    _fields_ = [("type", vp), ("from_", vp), ("term", vp), ("index", vp), ("log_term", vp),
                ("commit", vp), ("msg_runs", u32), ("reserved", u32), ("ent_len", vp),
                ("ent_term", vp)]


class QeFollowerOut(C.Structure):
    _fields_ = [("result", vp), ("resp_index", vp), ("reject_hint", vp), ("resp_log_term", vp),
                ("append_from", vp), ("events", vp)]


# qe_vote_step
QE_VMSG_NONE, QE_VMSG_VOTE, QE_VMSG_PREVOTE, QE_VMSG_VOTE_RESP = 0, 1, 2, 3
QE_VMSG_PREVOTE_RESP, QE_VMSG_HUP, QE_VMSG_TIMEOUT_NOW = 4, 5, 6
QE_VMF_FORCE, QE_VMF_REJECT = 1, 2
QE_VOTE_CHECK_QUORUM, QE_VOTE_PREVOTE = 1, 2
QE_VR_NONE, QE_VR_IGNORED, QE_VR_IN_LEASE, QE_VR_GRANT, QE_VR_REJECT = 0, 1, 2, 3, 4
QE_VR_STEPPED_DOWN, QE_VR_PENDING, QE_VR_LOST = 5, 6, 7
QE_VR_CAMPAIGN_PREVOTE, QE_VR_CAMPAIGN_VOTE, QE_VR_WON = 8, 9, 10
QE_VR_REFUSED = 16  # results >= this: nothing of the group changed
QE_VR_BAD_MSG = 16


class QeVoter(C.Structure):
    _fields_ = [("timer", vp), ("election_timeout", u32), ("flags", u32), ("voted", vp),
                ("granted", vp), ("no_campaign", vp)]


class QeVoteMsgs(C.Structure):
    _fields_ = [("type", vp), ("from_", vp), ("term", vp), ("index", vp), ("log_term", vp),
                ("flags", vp)]


class QeVoteOut(C.Structure):
    _fields_ = [("result", vp), ("resp_term", vp), ("req_log_term", vp), ("req_to", vp),
                ("elected", vp), ("events", vp)]


# qe_compact
QE_CP_NONE, QE_CP_CREATED, QE_CP_COMPACTED, QE_CP_SNAP_OUT_OF_DATE, QE_CP_ALREADY = 0, 1, 2, 4, 8
QE_CP_REFUSED = 16  # results >= this: nothing of the group changed
QE_CP_OUT_OF_BOUND, QE_CP_PAST_APPLIED = 16, 17
QE_STAT_COMPACTED = 2  # = QE_STAT_COMMIT_SUM


class QeCompaction(C.Structure):
    _fields_ = [("compact_index", vp), ("create_index", vp), ("applied", vp), ("snap_term", vp),
                ("result", vp)]


# qe_snapshot_step
QE_SMSG_NONE, QE_SMSG_SNAP = 0, 1
QE_SR_NONE, QE_SR_IGNORED, QE_SR_STALE, QE_SR_NOT_MEMBER = 0, 1, 2, 3
QE_SR_FAST_FORWARD, QE_SR_RESTORED = 4, 5
QE_SR_REFUSED = 16  # results >= this: nothing of the group changed
QE_SR_BAD_MSG, QE_SR_COMMIT_PAST_LOG, QE_SR_BAD_CONF = 16, 17, 18


class QeSnapMsgs(C.Structure):
    _fields_ = [("type", vp), ("from_", vp), ("term", vp), ("snap_index", vp), ("snap_term", vp),
                ("cs_inc", vp), ("cs_out", vp), ("cs_learner", vp), ("cs_learners_next", vp),
                ("cs_auto_leave", vp), ("cs_ids", vp)]


class QeSnapOut(C.Structure):
    _fields_ = [("result", vp), ("resp_index", vp), ("events", vp)]


# qe_outbox
QE_OMSG_APP, QE_OMSG_SNAP, QE_OMSG_HEARTBEAT, QE_OMSG_BAD = 1, 2, 3, 255
QE_STAT_OUTBOX_ENTRIES = 2    # = QE_STAT_COMMIT_SUM
QE_STAT_OUTBOX_APP, QE_STAT_OUTBOX_SNAP, QE_STAT_OUTBOX_HEARTBEAT = 4, 5, 6  # = QE_STAT_VOTE_*
QE_STAT_OUTBOX_BAD = 8        # = QE_STAT_REJECTED


class QeOutboxIn(C.Structure):
    _fields_ = [("sent", vp), ("snap", vp), ("hb_sent", vp), ("index", vp), ("next_before", vp),
                ("term", vp), ("snap_term", vp), ("hb_commit", vp), ("hb_ctx", vp),
                ("max_entries", u32), ("reserved", u32)]


class QeOutboxOut(C.Structure):
    _fields_ = [("capacity", u64), ("msg_runs", u32), ("reserved", u32), ("group", vp),
                ("to", vp), ("type", vp), ("term", vp), ("index", vp), ("log_term", vp),
                ("commit", vp), ("ctx", vp), ("ent_len", vp), ("ent_term", vp), ("count", vp)]


# qe_inbox
QE_IMSG_APP, QE_IMSG_SNAP, QE_IMSG_HEARTBEAT = 1, 2, 3   # = QE_OMSG_*
(QE_IMSG_APP_RESP, QE_IMSG_APP_RESP_REJECT, QE_IMSG_HEARTBEAT_RESP, QE_IMSG_SNAP_STATUS,
 QE_IMSG_SNAP_STATUS_REJECT, QE_IMSG_UNREACHABLE, QE_IMSG_TRANSFER_LEADER) = range(4, 11)
(QE_IMSG_VOTE, QE_IMSG_PREVOTE, QE_IMSG_VOTE_RESP, QE_IMSG_PREVOTE_RESP, QE_IMSG_TIMEOUT_NOW,
 QE_IMSG_HUP) = range(11, 17)
(QE_ID_ROUTED, QE_ID_STEPDOWN, QE_ID_DEFERRED, QE_ID_DROP_LOWER_TERM,
 QE_ID_DROP_NOT_LEADER) = range(1, 6)
QE_ID_BAD = 255
QE_INBOX_SRC_TICK = 0xFFFFFFFF
QE_STAT_INBOX_BAD = 1          # = QE_STAT_COMMIT_INF
QE_STAT_INBOX_ROUTED, QE_STAT_INBOX_LOWER_TERM, QE_STAT_INBOX_DEFERRED = 4, 5, 6  # = QE_STAT_VOTE_*
QE_STAT_INBOX_NOT_LEADER = 8   # = QE_STAT_REJECTED
QE_STAT_INBOX_STEPDOWN = 13    # = QE_STAT_STEPDOWNS


class QeInboxIn(C.Structure):
    _fields_ = [("num_records", u64), ("msg_runs", u32), ("reserved", u32), ("group", vp),
                ("from_", vp), ("type", vp), ("term", vp), ("index", vp), ("log_term", vp),
                ("commit", vp), ("hint", vp), ("ctx", vp), ("flags", vp), ("ent_len", vp),
                ("ent_term", vp), ("tick_action", vp)]


class QeInboxOut(C.Structure):
    _fields_ = [(k, vp) for k in (
        "f_type", "f_from", "f_term", "f_index", "f_log_term", "f_commit", "f_ent_len",
        "f_ent_term", "s_type", "s_from", "s_term", "s_snap_index", "s_snap_term", "v_type",
        "v_from", "v_term", "v_index", "v_log_term", "v_flags", "r_type", "r_index", "r_hint",
        "r_log_term", "r_ctx", "f_src", "s_src", "v_src", "r_src", "disposition", "deferred",
        "deferred_count")]


# qe_replies
QE_RMSG_BAD = 255
QE_STAT_REPLY_APP_RESP, QE_STAT_REPLY_HEARTBEAT_RESP = 4, 6   # = QE_STAT_VOTE_WON / _PENDING
QE_STAT_REPLY_VOTE_RESP, QE_STAT_REPLY_BAD = 7, 8             # = QE_STAT_GRANTED / _REJECTED
QE_STAT_REPLY_VOTE_REQ, QE_STAT_REPLY_TIMEOUT_NOW = 11, 12    # = QE_STAT_ELECTIONS / _LEADERS


class QeRepliesIn(C.Structure):
    _fields_ = [(k, vp) for k in (
        "term", "f_result", "f_from", "f_resp_index", "f_reject_hint", "f_resp_log_term", "f_ctx",
        "s_result", "s_from", "s_resp_index", "v_result", "v_type", "v_from", "v_resp_term",
        "v_req_log_term", "v_req_to", "timeout_now")] + [("reserved", u32 * 2)]


class QeRepliesOut(C.Structure):
    _fields_ = [("capacity", u64)] + [(k, vp) for k in (
        "group", "to", "type", "term", "index", "log_term", "hint", "ctx", "flags", "count")]


# qe_carry
QE_PEER_NONE = 0xFFFFFFFFFFFFFFFF
QE_CARRY_SNAP_STATUS = 1
QE_CARRY_TYPES = 0xFC7E        # the carriable types 1..6 and 10..15, as `ignore` bits
QE_TD_LOCAL, QE_TD_REMOTE, QE_TD_LOST = 1, 2, 3
QE_TD_BAD = 255
QE_STAT_CARRY_BAD = 1          # = QE_STAT_COMMIT_INF
QE_STAT_CARRY_LOCAL, QE_STAT_CARRY_LOST, QE_STAT_CARRY_REMOTE = 4, 5, 6   # = QE_STAT_VOTE_*
QE_STAT_CARRY_SNAP_STATUS = 9  # = QE_STAT_COMMIT_ADVANCED


class QePeers(C.Structure):
    _fields_ = [("peer_group", vp), ("peer_from", vp)]


class QeCarryIn(C.Structure):
    _fields_ = [("capacity", u64), ("count", vp), ("msg_runs", u32), ("flags", u32)] + [
        (k, vp) for k in ("group", "to", "type", "term", "index", "log_term", "commit", "hint",
                          "ctx", "mflags", "ent_len", "ent_term", "drop", "cut")] + [
        ("ignore", u32), ("reserved", u32)]


class QeCarryOut(C.Structure):
    _fields_ = [("capacity", u64), ("base", u64), ("ent_pitch", u64), ("msg_runs", u32),
                ("reserved", u32)] + [(k, vp) for k in (
                    "group", "from_", "type", "term", "index", "log_term", "commit", "hint", "ctx",
                    "mflags", "ent_len", "ent_term", "src", "count", "disposition", "remote",
                    "remote_count")]


# qe_ready_note / qe_ready / qe_advance
QE_RD_SOFT, QE_RD_HARD, QE_RD_MUST_SYNC, QE_RD_SNAP, QE_RD_ENTS_CUT, QE_RD_APPLY_CUT = (
    1, 2, 4, 8, 16, 32)
QE_ADV_OK, QE_ADV_OK_STALE_ENTRIES = 1, 2
QE_ADV_REFUSED = 8  # outcomes >= this: nothing of the group changed
QE_ADV_BAD_GROUP, QE_ADV_APPLIED_RANGE = 8, 9
QE_ADV_OUTCOME, QE_ADV_AUTO_LEAVE = 0x0F, 0x10
QE_STAT_READY_ENTRIES = 2     # = QE_STAT_COMMIT_SUM
QE_STAT_READY_MUST_SYNC = 4   # = QE_STAT_VOTE_WON
QE_STAT_READY_APPLY = 9       # = QE_STAT_COMMIT_ADVANCED


class QeReadyState(C.Structure):
    _fields_ = [(k, vp) for k in (
        "stable", "applied", "snap_pending", "prev_term", "prev_commit", "prev_vote", "prev_lead",
        "prev_state")]


class QeReadyNoteIn(C.Structure):
    _fields_ = [(k, vp) for k in ("follow_result", "append_from", "snap_result",
                                  "snap_resp_index")]


class QeReadyIn(C.Structure):
    _fields_ = [("pending", vp), ("max_apply", u32), ("reserved", u32)]


class QeReadyOut(C.Structure):
    _fields_ = [("capacity", u64), ("ent_runs", u32), ("reserved", u32)] + [(k, vp) for k in (
        "group", "term", "commit", "vote", "lead", "state", "flags", "ent_first", "ent_count",
        "ent_last_term", "apply_first", "apply_count", "snap_index", "ent_len", "ent_term",
        "apply_len", "apply_term", "count")]


class QeAdvanceOpt(C.Structure):
    _fields_ = [("auto_leave", vp), ("pending_conf_index", vp), ("reserved", u32 * 2)]


# qe_read_note / qe_read_states
QE_RS_STATE, QE_RS_RESP, QE_RS_TERM_COMMIT = 1, 2, 3
QE_STAT_READ_STATE, QE_STAT_READ_RESP = 4, 6   # = QE_STAT_VOTE_WON / _PENDING
QE_STAT_READ_TERM_COMMIT = 9                   # = QE_STAT_COMMIT_ADVANCED


class QeReadBook(C.Structure):
    _fields_ = [("req_index", vp), ("req_from", vp)]


class QeReadStatesIn(C.Structure):
    _fields_ = [(k, vp) for k in (
        "read_released", "term_commit", "term_commit_index", "ri_result", "ri_index", "ri_from",
        "ri_key")] + [("reserved", u32 * 2)]


class QeReadStatesOut(C.Structure):
    _fields_ = [("capacity", u64)] + [(k, vp) for k in (
        "group", "kind", "to", "ctx", "index", "key", "count")]


# qe_requests
QE_QMSG_TRANSFER_LEADER = 10   # = QE_IMSG_TRANSFER_LEADER
QE_QMSG_PROP, QE_QMSG_READ_INDEX, QE_QMSG_READ_INDEX_RESP = 17, 18, 19
(QE_QD_ROUTED, QE_QD_STEPDOWN, QE_QD_DEFERRED, QE_QD_DROP_LOWER_TERM, QE_QD_NO_ARM,
 QE_QD_FORWARDED, QE_QD_READ_STATE, QE_QD_PROP_DROPPED, QE_QD_NO_LEADER,
 QE_QD_REF_PANIC) = range(1, 11)
QE_QD_BAD = 255
QE_QO_FWD, QE_QO_READ_STATE, QE_QO_PROP_DROPPED = 1, 2, 3
QE_REQ_NO_FORWARD = 1
QE_STAT_REQ_BAD, QE_STAT_REQ_NO_ARM, QE_STAT_REQ_NO_LEADER = 1, 2, 3   # = QE_STAT_COMMIT_*
QE_STAT_REQ_ROUTED, QE_STAT_REQ_LOWER_TERM, QE_STAT_REQ_DEFERRED = 4, 5, 6  # = QE_STAT_VOTE_*
QE_STAT_REQ_FORWARDED, QE_STAT_REQ_PROP_DROPPED = 7, 8   # = QE_STAT_GRANTED / _REJECTED
QE_STAT_REQ_READ_STATE = 9     # = QE_STAT_COMMIT_ADVANCED
QE_STAT_REQ_REF_PANIC = 10     # = QE_STAT_READ_RELEASED
QE_STAT_REQ_STEPDOWN = 13      # = QE_STAT_STEPDOWNS


class QeRequestsIn(C.Structure):
    _fields_ = [("num_records", u64), ("max_cc", u32), ("flags", u32)] + [(k, vp) for k in (
        "group", "type", "from_", "term", "index", "key", "num_entries", "payload", "cc_count",
        "cc_pos", "cc_leave", "cc_size")] + [("reserved", u64)]


class QeRequestsOut(C.Structure):
    _fields_ = [(k, vp) for k in (
        "p_num_entries", "p_payload", "p_cc_count", "p_cc_pos", "p_cc_leave", "p_cc_size")] + [
        ("cc_stride", u64)] + [(k, vp) for k in (
            "ri_request", "ri_key", "ri_from", "v_type", "v_from", "v_term", "v_index",
            "v_log_term", "v_flags", "r_type", "p_src", "ri_src", "v_src", "r_src", "disposition",
            "deferred", "deferred_count")] + [("capacity", u64)] + [(k, vp) for k in (
                "group", "kind", "type", "to", "from_", "term", "index", "key", "src", "count")]


# qe_apply_conf
QE_AC_AUTO, QE_AC_JOINT_IMPLICIT, QE_AC_JOINT_EXPLICIT = 0, 1, 2   # ConfChangeTransition
QE_AC_ANY_SLOT = 0xFF
QE_AC_APPLIED, QE_AC_LEADER, QE_AC_DEFERRED = 1, 2, 3
QE_AC_REFUSED = 16  # results >= this: nothing of the group written
(QE_AC_BAD_GROUP, QE_AC_BAD_ORDER, QE_AC_BAD_CHANGE, QE_AC_CHANGER_ERROR,
 QE_AC_SKIPPED) = range(16, 21)
(QE_CC_OK, QE_CC_ERR_INVARIANT, QE_CC_ERR_ALREADY_JOINT, QE_CC_ERR_ZERO_VOTER_JOINT,
 QE_CC_ERR_NOT_JOINT, QE_CC_ERR_SIMPLE_IN_JOINT, QE_CC_ERR_BAD_TYPE, QE_CC_ERR_REMOVED_ALL,
 QE_CC_ERR_SIMPLE_MULTI, QE_CC_ERR_INVARIANT_OUT, QE_CC_ERR_NO_SLOT) = range(11)


class QeApplyConfIn(C.Structure):
    _fields_ = [("capacity", u64), ("n", u64), ("count", vp), ("max_changes", u32),
                ("reserved", u32)] + [(k, vp) for k in (
                    "group", "transition", "num_changes", "type", "node_id", "slot")]


class QeApplyConfOut(C.Structure):
    _fields_ = [(k, vp) for k in (
        "result", "cc_result", "sw_result", "inc", "out", "learner", "learners_next", "tracked",
        "new_progress", "auto_leave", "ids")]


QE_BL_NONE, QE_BL_LEADER, QE_BL_NOT_MEMBER, QE_BL_RUNS_FULL = 0, 1, 2, 3
QE_BL_BCAST = 1

QE_SW_NONE, QE_SW_REMOVED, QE_SW_NO_VOTERS, QE_SW_BCAST, QE_SW_PROBE = 0, 1, 2, 3, 4
QE_SW_OUTCOME, QE_SW_TRANSFER_ABORTED = 0x0F, 0x10

QE_PROP_NONE, QE_PROP_OK, QE_PROP_DROPPED_NOT_MEMBER, QE_PROP_DROPPED_TRANSFER, \
    QE_PROP_DROPPED_SIZE = 0, 1, 2, 3, 4
QE_PROP_BAD_CC = 5  # ABI 7: more conf-change entries than max_cc
QE_PROP_MAX_CC = 8
QE_PROP_APPEND_ONLY = 1

QE_PR_PROBE, QE_PR_REPLICATE, QE_PR_SNAPSHOT = 0, 1, 2
QE_PF_STATE, QE_PF_PROBE_SENT, QE_PF_RECENT_ACTIVE = 3, 4, 8
QE_PW_START_SHIFT, QE_PW_COUNT_SHIFT = 8, 16
QE_PF_RING_WIDE = 16
QE_PW_RING_MASK = 0xFF0000F0  # ring representation bits (ABI 4), not Progress state
QE_RING_EPOCH_MAX = 0x7FF


def QE_RING_PITCH(F):
    return (int(F) + 3) & ~3
QE_MSG_NONE, QE_MSG_APP_RESP, QE_MSG_APP_RESP_REJECT, QE_MSG_HEARTBEAT_RESP = 0, 1, 2, 3
QE_MSG_SNAP_STATUS, QE_MSG_SNAP_STATUS_REJECT, QE_MSG_UNREACHABLE = 4, 5, 6
QE_MSG_TRANSFER_LEADER = 7  # ABI 5
QE_READ_QUEUE = 4           # ABI 5: ReadIndex requests pending per group
QE_RI_NONE, QE_RI_RESPOND, QE_RI_POSTPONED, QE_RI_QUEUED, QE_RI_FULL = 0, 1, 2, 3, 4
QE_RI_DUPLICATE = 5         # ABI 7: the request's key is pending already
QE_READ_CAP_MAX = 255       # ABI 7: the longest queue (read_cap)
QE_RING16_MAX_F = 8         # ABI 8: the 16-bit Inflights form (infl16)
QE_RING16_MAX_SLOTS = 9
QE_MAX_INFLIGHT = 255
QE_MAX_LOG_RUNS = 16

QE_PACK_TOO_MANY_PEERS = 1
QE_PACK_LEARNER_IS_VOTER = 2
QE_PACK_LEARNER_NEXT_NOT_OUTGOING = 4
QE_PACK_ZERO_ID = 8


class QeConf(C.Structure):
    _fields_ = [
        ("num_groups", u64), ("num_slots", u32), ("reserved", u32), ("slot_ids", vp),
        ("inc_mask", vp), ("out_mask", vp), ("learner_mask", vp), ("learners_next_mask", vp),
        ("is_learner", vp), ("tracked", vp), ("auto_leave", vp),
    ]


class QeConfChanges(C.Structure):
    _fields_ = [
        ("max_changes", u32), ("reserved", u32), ("stride", u64), ("op", vp), ("count", vp),
        ("type", vp), ("node_id", vp), ("last_index", vp), ("result", vp),
        ("new_progress", vp),
    ]


QE_CC_ADD_NODE, QE_CC_REMOVE_NODE, QE_CC_UPDATE_NODE, QE_CC_ADD_LEARNER_NODE = 0, 1, 2, 3
QE_CC_OP_NONE, QE_CC_OP_SIMPLE, QE_CC_OP_ENTER_JOINT, QE_CC_OP_ENTER_JOINT_AUTO, \
    QE_CC_OP_LEAVE_JOINT = 0, 1, 2, 3, 4


# Every symbol include/etcd_quorum.h declares, with its prototype.
PROTOTYPES = {
    "qe_abi_version": (C.c_int, []),
    "qe_strerror": (C.c_char_p, [C.c_int]),
    "qe_mask_bytes": (C.c_size_t, [u32]),
    "qe_tune": (C.c_int, [C.c_char_p, C.c_int]),
    "qe_commit_vote": (C.c_int, [C.POINTER(QeGroups), C.POINTER(QeOutputs), vp]),
    "qe_committed_index": (C.c_int, [C.POINTER(QeGroups), vp, vp]),
    "qe_vote_result": (C.c_int, [C.POINTER(QeGroups), vp, vp]),
    "qe_quorum_active": (C.c_int, [C.POINTER(QeGroups), vp, vp, vp]),
    "qe_record_votes": (C.c_int, [u64, u32, vp, vp, vp, vp, vp]),
    "qe_replication_round": (C.c_int, [C.POINTER(QeReplState), C.POINTER(QeReplMsgs), vp, vp]),
    "qe_election_steps": (C.c_int, [C.POINTER(QeElectionState), C.POINTER(QeElectionParams),
                                    vp, vp]),
    "qe_stats_reduce": (C.c_int, [vp, vp, vp]),
    "qe_collect_scratch_bytes": (C.c_size_t, [u64]),
    "qe_collect": (C.c_int, [u64, u64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "qe_outbox_scratch_bytes": (C.c_size_t, [u64]),
    "qe_outbox": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeOutboxIn), C.POINTER(QeOutboxOut),
                            vp, vp, vp]),
    "qe_inbox_scratch_bytes": (C.c_size_t, [u64, u32, u64]),
    "qe_inbox": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower), C.POINTER(QeInboxIn),
                           C.POINTER(QeInboxOut), vp, vp, vp]),
    "qe_replies_scratch_bytes": (C.c_size_t, [u64]),
    "qe_replies": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeRepliesIn),
                             C.POINTER(QeRepliesOut), vp, vp, vp]),
    "qe_carry_scratch_bytes": (C.c_size_t, [u64]),
    "qe_carry": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QePeers), C.POINTER(QeCarryIn),
                           C.POINTER(QeCarryOut), vp, vp, vp]),
    "qe_ready_note": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeReadyState),
                                C.POINTER(QeReadyNoteIn), vp]),
    "qe_ready_scratch_bytes": (C.c_size_t, [u64]),
    "qe_ready": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower), C.POINTER(QeReadyState),
                           C.POINTER(QeReadyIn), C.POINTER(QeReadyOut), vp, vp, vp]),
    "qe_advance": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower),
                             C.POINTER(QeReadyState), C.POINTER(QeReadyOut),
                             C.POINTER(QeAdvanceOpt), vp, vp]),
    "qe_read_note": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeReadBook), vp, vp, vp, vp, vp]),
    "qe_read_states_scratch_bytes": (C.c_size_t, [u64]),
    "qe_read_states": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeReadBook),
                                 C.POINTER(QeReadStatesIn), C.POINTER(QeReadStatesOut), vp, vp,
                                 vp]),
    "qe_requests_scratch_bytes": (C.c_size_t, [u64, u64]),
    "qe_requests": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower),
                              C.POINTER(QeRequestsIn), C.POINTER(QeRequestsOut), vp, vp, vp]),
    "qe_apply_conf_scratch_bytes": (C.c_size_t, [u64]),
    "qe_apply_conf": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower), C.POINTER(QeConf),
                                C.POINTER(QeApplyConfIn), C.POINTER(QeApplyConfOut),
                                C.POINTER(QeSwitch), vp, vp]),
    "qe_gen_groups": (C.c_int, [C.POINTER(QeGroups), C.POINTER(QeGenParams), vp]),
    "qe_apply_append_resps": (C.c_int, [u64, u32, u64, vp, vp, u64, vp, vp, vp, vp, vp]),
    "qe_pack_confstate": (C.c_int, [C.POINTER(QeConfStateCSR), u32, vp, vp, vp, vp, vp, vp]),
    "qe_pack_conf": (C.c_int, [C.POINTER(QeConfStateCSR), C.POINTER(QeConf), vp, vp]),
    "qe_pack_order": (C.c_int, [C.POINTER(QeConfStateCSR), u32, vp, vp]),
    "qe_pack_match": (C.c_int, [u64, u32, vp, vp, vp, vp, vp, vp, u64, vp]),
    "qe_pack_votes": (C.c_int, [u64, u32, vp, vp, vp, vp, vp, vp, vp]),
    "qe_slot_lookup": (C.c_int, [u64, u32, vp, u64, vp, vp, vp]),
    "qe_pack_threads": (C.c_int, [C.c_int]),
    "qe_progress_step": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QePeerMsgs), vp, vp]),
    "qe_progress_send": (C.c_int, [C.POINTER(QeProgress), vp, u32, vp, vp, vp]),
    "qe_check_quorum": (C.c_int, [C.POINTER(QeProgress), vp, vp, vp]),
    "qe_read_index": (C.c_int, [C.POINTER(QeProgress), vp, vp, u32, vp, vp, vp, vp]),
    "qe_propose": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeProposals), vp, vp]),
    "qe_heartbeat": (C.c_int, [C.POINTER(QeProgress), vp, vp, vp, vp]),
    "qe_tick": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeTimers), C.POINTER(QeTickOut), vp,
                          vp]),
    "qe_follower_step": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower),
                                   C.POINTER(QeLeaderMsgs), C.POINTER(QeFollowerOut), vp, vp]),
    "qe_vote_step": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower), C.POINTER(QeVoter),
                               C.POINTER(QeVoteMsgs), C.POINTER(QeVoteOut), vp, vp]),
    "qe_compact": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeCompaction), vp, vp]),
    "qe_snapshot_step": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeFollower),
                                   C.POINTER(QeConf), C.POINTER(QeSnapMsgs),
                                   C.POINTER(QeSnapOut), vp, vp]),
    "qe_switch_config": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeSwitch), vp, vp]),
    "qe_become_leader": (C.c_int, [C.POINTER(QeProgress), C.POINTER(QeLeader), vp, vp]),
    "qe_ring_pack": (C.c_int, [u64, u32, u32, u64, vp, vp, vp, vp]),
    "qe_ring_unpack": (C.c_int, [u64, u32, u32, u64, vp, vp, vp, vp]),
    "qe_ring_pack16": (C.c_int, [u64, u32, u32, u64, vp, vp, vp, vp, vp, vp]),
    "qe_ring_unpack16": (C.c_int, [u64, u32, u32, u64, vp, vp, vp, vp, vp, vp]),
    "qe_confchange": (C.c_int, [C.POINTER(QeConf), C.POINTER(QeConfChanges),
                                C.POINTER(QeProgress), vp]),
    "qe_comm_id_bytes": (C.c_size_t, []),
    "qe_comm_unique_id": (C.c_int, [vp]),
    "qe_comm_init": (C.c_int, [C.POINTER(vp), u32, u32, vp, C.c_int]),
    "qe_comm_init_timeout": (C.c_int, [C.POINTER(vp), u32, u32, vp, C.c_int, u32]),
    "qe_comm_destroy": (C.c_int, [vp]),
    "qe_comm_abort": (C.c_int, [vp]),
    "qe_allreduce_stats": (C.c_int, [vp, u32, vp, vp]),
}


class QuorumEngineError(RuntimeError):
    def __init__(self, fn, status):
        msg = _LIB.qe_strerror(status).decode() if _LIB is not None else str(status)
        super().__init__(f"{fn} failed: {status} ({msg})")
        self.status = status


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"etcd_amd: HIP library {LIB_PATH} is missing; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if lib.qe_abi_version() != QE_ABI_VERSION:
        raise ImportError("etcd_amd: ABI version mismatch")
    return lib


_LIB = None
_LIB = _load()


def lib():
    return _LIB


def check(fn, status):
    if status != QE_OK:
        raise QuorumEngineError(fn, status)
    return status
