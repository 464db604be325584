"""qe_replies restated in plain Python (include/etcd_quorum.h states the rules):
the result rows and masks of the receiver-side calls -> the ordered list of
message records and the statistics.  Imports no torch.

`st` carries what the call reads of qe_progress (num_groups, group_offset,
num_slots, stride, last_index), `inp` the fields of qe_replies_in; a row that
is not given is None.  Rows are flat sequences indexed [g]."""
from types import SimpleNamespace

# QE_IMSG_*
APP_RESP, APP_RESP_REJECT, HEARTBEAT_RESP = 4, 5, 6
VOTE, PREVOTE, VOTE_RESP, PREVOTE_RESP, TIMEOUT_NOW = 11, 12, 13, 14, 15
BAD = 255
FR_LOWER_TERM_RESP, FR_HEARTBEAT_RESP, FR_APP_ACCEPT, FR_APP_REJECT, FR_APP_STALE = 2, 3, 4, 5, 6
SR_STALE, SR_NOT_MEMBER, SR_FAST_FORWARD, SR_RESTORED = 2, 3, 4, 5
VR_GRANT, VR_REJECT, VR_CAMPAIGN_PREVOTE, VR_CAMPAIGN_VOTE = 3, 4, 8, 9
VMSG_VOTE, VMSG_PREVOTE, VMSG_TIMEOUT_NOW = 1, 2, 6
VMF_FORCE, VMF_REJECT = 1, 2
M64 = (1 << 64) - 1
PHI, SALT = 0x9E3779B97F4A7C15, 0xA0761D6478BD642F
STAT_GROUPS, STAT_APP_RESP, STAT_HEARTBEAT_RESP, STAT_VOTE_RESP, STAT_BAD = 0, 4, 6, 7, 8
STAT_VOTE_REQ, STAT_TIMEOUT_NOW, STAT_VIOLATIONS, STAT_CHECKSUM = 11, 12, 14, 15
BY_TYPE = {APP_RESP: STAT_APP_RESP, APP_RESP_REJECT: STAT_APP_RESP,
           HEARTBEAT_RESP: STAT_HEARTBEAT_RESP, VOTE_RESP: STAT_VOTE_RESP,
           PREVOTE_RESP: STAT_VOTE_RESP, VOTE: STAT_VOTE_REQ, PREVOTE: STAT_VOTE_REQ,
           TIMEOUT_NOW: STAT_TIMEOUT_NOW, BAD: STAT_BAD}
FIELDS = ("group", "to", "type", "term", "index", "log_term", "hint", "ctx", "flags")
KINDS = ("F", "S", "VR", "VQ", "T")


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def state(**kw):
    d = dict(num_groups=0, group_offset=0, num_slots=1, stride=0, last_index=None)
    d.update(kw)
    return SimpleNamespace(**d)


def inputs(**kw):
    d = dict(term=None, f_result=None, f_from=None, f_resp_index=None, f_reject_hint=None,
             f_resp_log_term=None, f_ctx=None, s_result=None, s_from=None, s_resp_index=None,
             v_result=None, v_type=None, v_from=None, v_resp_term=None, v_req_log_term=None,
             v_req_to=None, timeout_now=None)
    d.update(kw)
    return SimpleNamespace(**d)


def rec(st, g, to, type, term, **kw):
    r = dict(group=st.group_offset + g, to=int(to), type=type, term=int(term), index=0, log_term=0,
             hint=0, ctx=0, flags=0)
    r.update({k: int(v) for k, v in kw.items()})
    return r


def single(st, r):
    """Rule 2: a single-`to` record whose `to` is no slot keeps group, to and
    term and nothing else."""
    if r["to"] >= st.num_slots or r["type"] == BAD:
        r = dict(r, type=BAD, index=0, log_term=0, hint=0, ctx=0, flags=0)
    return r


def group_records(st, inp, g, drop_hint=False):
    """-> {kind: the records of group g, by slot}."""
    full = (1 << st.num_slots) - 1
    out = {k: [] for k in KINDS}
    fr = int(inp.f_result[g]) if inp.f_result is not None else 0
    if FR_LOWER_TERM_RESP <= fr <= FR_APP_STALE:
        to, term = inp.f_from[g], inp.term[g]
        if fr == FR_LOWER_TERM_RESP:
            r = rec(st, g, to, APP_RESP, term)
        elif fr == FR_HEARTBEAT_RESP:
            r = rec(st, g, to, HEARTBEAT_RESP, term,
                    ctx=inp.f_ctx[g] if inp.f_ctx is not None else 0)
        elif fr == FR_APP_REJECT:
            r = rec(st, g, to, APP_RESP_REJECT, term, index=inp.f_resp_index[g],
                    hint=0 if drop_hint else inp.f_reject_hint[g], log_term=inp.f_resp_log_term[g])
        else:
            r = rec(st, g, to, APP_RESP, term, index=inp.f_resp_index[g])
        out["F"].append(single(st, r))
    sr = int(inp.s_result[g]) if inp.s_result is not None else 0
    if SR_STALE <= sr <= SR_RESTORED:
        out["S"].append(single(st, rec(st, g, inp.s_from[g], APP_RESP, inp.term[g],
                                       index=inp.s_resp_index[g])))
    vr = int(inp.v_result[g]) if inp.v_result is not None else 0
    if vr in (VR_GRANT, VR_REJECT):
        ty = {VMSG_VOTE: VOTE_RESP, VMSG_PREVOTE: PREVOTE_RESP}.get(int(inp.v_type[g]), BAD)
        out["VR"].append(single(st, rec(st, g, inp.v_from[g], ty, inp.v_resp_term[g],
                                        flags=VMF_REJECT if vr == VR_REJECT else 0)))
    elif vr in (VR_CAMPAIGN_VOTE, VR_CAMPAIGN_PREVOTE):
        force = vr == VR_CAMPAIGN_VOTE and int(inp.v_type[g]) == VMSG_TIMEOUT_NOW
        for s in range(st.num_slots):
            if (int(inp.v_req_to[g]) & full) >> s & 1:
                out["VQ"].append(rec(st, g, s, VOTE if vr == VR_CAMPAIGN_VOTE else PREVOTE,
                                     inp.v_resp_term[g], index=st.last_index[g],
                                     log_term=inp.v_req_log_term[g],
                                     flags=VMF_FORCE if force else 0))
    if inp.timeout_now is not None:
        for s in range(st.num_slots):
            if (int(inp.timeout_now[g]) & full) >> s & 1:
                out["T"].append(rec(st, g, s, TIMEOUT_NOW, inp.term[g]))
    return out


def build(st, inp, drop_hint=False):
    """-> (records in list order, stats as {counter index: value}).
    drop_hint=True leaves the RejectHint out of reject records (a negative
    control)."""
    recs, groups = [], 0
    for t0 in range(0, st.num_groups, 64):
        tile = {g: group_records(st, inp, g, drop_hint)
                for g in range(t0, min(st.num_groups, t0 + 64))}
        groups += sum(1 for by in tile.values() if any(by.values()))
        for kind in ("F", "S", "VR"):
            for g in tile:
                recs += tile[g][kind]
        for kind in ("VQ", "T"):
            for s in range(st.num_slots):
                for g in tile:
                    recs += [r for r in tile[g][kind] if r["to"] == s]
    stats = {k: 0 for k in set(BY_TYPE.values()) | {STAT_GROUPS, STAT_VIOLATIONS, STAT_CHECKSUM}}
    stats[STAT_GROUPS] = groups
    for r in recs:
        stats[BY_TYPE[r["type"]]] += 1
        stats[STAT_VIOLATIONS] += r["type"] == BAD
        h = mix64((r["group"] * PHI) ^ SALT ^ (r["type"] << 56) ^ (r["to"] << 48))
        for x in (r["term"], r["index"], r["log_term"], r["hint"], r["ctx"] | r["flags"] << 32):
            h = mix64(h ^ x)
        stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
    return recs, stats


def truncate(recs, capacity):
    """What the arrays hold: the first min(count, capacity) records."""
    return len(recs), recs[:capacity]
