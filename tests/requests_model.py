"""qe_requests restated in plain Python (include/etcd_quorum.h states the rules
1-6): a list of client requests in arrival order handled as raft.Step would on
each record's receiver -> the leader-side rows of one pass of calls, a
disposition per record, the deferred list, the output list and the statistics.
This is the SEQUENTIAL rule, one plain loop over the list; the kernels compute
it in an order-free form, which route_by_stop() restates.  Imports no torch.

A record is a dict: group (the receiver's global id), type (QMSG), from (a slot
or NONE), term, index, key, num_entries, payload, cc [(pos, leave, size), ...].
`st` carries num_groups, group_offset, num_slots and the rows term[G], state[G],
lead[G] of qe_follower and self_slot[G] of qe_progress."""
from types import SimpleNamespace

from tests.inbox_model import record_hashes as inbox_hashes

TRANSFER_LEADER, PROP, READ_INDEX, READ_INDEX_RESP = 10, 17, 18, 19
TYPES = (TRANSFER_LEADER, PROP, READ_INDEX, READ_INDEX_RESP)
NONE = 0xFF
(ROUTED, STEPDOWN, DEFERRED, DROP_LOWER_TERM, NO_ARM, FORWARDED, READ_STATE, PROP_DROPPED,
 NO_LEADER, REF_PANIC) = range(1, 11)
BAD = 255
QD_NAMES = {1: "ROUTED", 2: "STEPDOWN", 3: "DEFERRED", 4: "DROP_LOWER_TERM", 5: "NO_ARM",
            6: "FORWARDED", 7: "READ_STATE", 8: "PROP_DROPPED", 9: "NO_LEADER", 10: "REF_PANIC",
            255: "BAD"}
QO_FWD, QO_READ_STATE, QO_PROP_DROPPED = 1, 2, 3
ST_FOLLOWER, ST_CANDIDATE, ST_LEADER, ST_PRE_CANDIDATE = 0, 1, 2, 3
MSG_TRANSFER_LEADER, VMSG_VOTE_RESP, VMF_REJECT = 7, 3, 2
M64 = (1 << 64) - 1
PHI, SALT = 0x9E3779B97F4A7C15, 0xA24BAED4963EE407
STAT_GROUPS, STAT_VIOLATIONS, STAT_CHECKSUM = 0, 14, 15
BY_DISPOSITION = {BAD: 1, NO_ARM: 2, NO_LEADER: 3, ROUTED: 4, DROP_LOWER_TERM: 5, DEFERRED: 6,
                  FORWARDED: 7, PROP_DROPPED: 8, READ_STATE: 9, REF_PANIC: 10, STEPDOWN: 13}


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def record_hash(group, disp, type, frm, i):
    """The STAT_CHECKSUM term of record i of the list."""
    h = mix64((group * PHI) ^ SALT ^ (disp << 56) ^ (type << 48) ^ (frm << 40))
    return mix64(h ^ i)


def record_hashes(group, disp, type, frm):
    """record_hash over the arrays of a whole list (position = array index),
    vectorised -> uint64[n]; tests/test_requests_model.py pins it to the scalar
    form."""
    return inbox_hashes(group, disp, type, frm, SALT)


def rec(group, type, frm=NONE, term=0, index=0, key=0, num_entries=0, payload=0, cc=()):
    return {"group": int(group), "type": int(type), "from": int(frm), "term": int(term),
            "index": int(index), "key": int(key), "num_entries": int(num_entries),
            "payload": int(payload), "cc": [(int(p), int(l), int(s)) for p, l, s in cc]}


def state(**kw):
    d = dict(num_groups=0, group_offset=0, num_slots=1, term=None, state=None, lead=None,
             self_slot=None)
    d.update(kw)
    return SimpleNamespace(**d)


def is_bad(st, m):
    """Rule 1."""
    g, S, t = m["group"] - st.group_offset, st.num_slots, m["type"]
    return (not 0 <= g < st.num_groups or t not in TYPES or
            not (m["from"] < S or m["from"] == NONE) or
            (t == PROP and m["num_entries"] == 0) or
            (t in (PROP, READ_INDEX) and m["term"] != 0) or
            (t == TRANSFER_LEADER and m["from"] == NONE))


def step(st, m, no_forward=False, fwd_without_lead=False):
    """Rules 2 and 3 for one record that is not BAD, on an open group ->
    (disposition, the kind of its output record or 0).  fwd_without_lead is a
    negative control: a proposal forwarded although lead is None."""
    g, S, t = m["group"] - st.group_offset, st.num_slots, m["type"]
    rterm, role, lead = int(st.term[g]), int(st.state[g]), int(st.lead[g])
    if m["term"] != 0 and m["term"] < rterm:
        return DROP_LOWER_TERM, 0
    if m["term"] != 0 and m["term"] > rterm:
        return STEPDOWN, QO_READ_STATE if t == READ_INDEX_RESP else 0
    if role == ST_LEADER:
        return (NO_ARM, 0) if t == READ_INDEX_RESP else (ROUTED, 0)
    if role in (ST_CANDIDATE, ST_PRE_CANDIDATE):
        return (PROP_DROPPED, QO_PROP_DROPPED) if t == PROP else (NO_ARM, 0)
    has_lead = lead < S
    if t == READ_INDEX_RESP:
        return READ_STATE, QO_READ_STATE
    if t == PROP:
        if (has_lead or fwd_without_lead) and not no_forward:
            return FORWARDED, QO_FWD
        return PROP_DROPPED, QO_PROP_DROPPED
    if not has_lead:
        return NO_LEADER, 0
    if t == TRANSFER_LEADER and m["term"] != 0:
        return REF_PANIC, 0
    return FORWARDED, QO_FWD


def out_record(st, m, kind, i, fwd_from_self=False):
    """Rule 5.  fwd_from_self is a negative control: forwarding with `from`
    overwritten by the forwarder's own slot."""
    g, t = m["group"] - st.group_offset, m["type"]
    fwd = kind == QO_FWD
    lead = int(st.lead[g])
    frm = NONE
    if fwd:
        frm = m["from"] if m["from"] < st.num_slots and not fwd_from_self else int(st.self_slot[g])
    return dict(group=m["group"], kind=kind, type=t,
                to=(lead if lead < st.num_slots else NONE) if fwd else NONE, frm=frm,
                term=int(st.term[g]) if fwd and t == TRANSFER_LEADER else 0,
                index=m["index"] if kind == QO_READ_STATE else 0, key=m["key"], src=i)


def _finish(st, recs, disp, kinds, max_cc, fwd_from_self=False):
    """The rows, the lists and the statistics from the dispositions."""
    n = len(recs)
    out = SimpleNamespace(p={}, ri={}, v={}, r={}, disposition=disp)
    for i, m in enumerate(recs):
        g = m["group"] - st.group_offset
        if disp[i] == ROUTED and m["type"] == PROP:
            cc = (list(m["cc"][:max_cc]) + [(0, 0, 0)] * max_cc)[:max_cc]
            out.p[g] = dict(num_entries=m["num_entries"], payload=m["payload"],
                            cc_count=len(m["cc"]), cc=cc, src=i)
        elif disp[i] == ROUTED and m["type"] == READ_INDEX:
            out.ri[g] = dict(key=m["key"], frm=m["from"], src=i)
        elif disp[i] == ROUTED:
            out.r[(m["from"], g)] = dict(type=MSG_TRANSFER_LEADER, src=i)
        elif disp[i] == STEPDOWN:
            out.v[g] = dict(type=VMSG_VOTE_RESP, frm=m["from"], term=m["term"], index=0,
                            log_term=0, flags=VMF_REJECT, src=i)
    out.deferred = [i for i in range(n) if disp[i] == DEFERRED]
    out.records = [out_record(st, recs[i], kinds[i], i, fwd_from_self) for i in range(n)
                   if kinds[i]]
    stats = {k: 0 for k in list(BY_DISPOSITION.values()) + [STAT_GROUPS, STAT_VIOLATIONS,
                                                            STAT_CHECKSUM]}
    stats[STAT_GROUPS] = len({recs[i]["group"] for i in range(n) if disp[i] == ROUTED})
    for i, m in enumerate(recs):
        stats[BY_DISPOSITION[disp[i]]] += 1
        stats[STAT_VIOLATIONS] += disp[i] in (BAD, REF_PANIC)
        h = record_hash(m["group"], disp[i], m["type"], m["from"], i)
        stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
    out.stats = stats
    return out


def route(st, recs, no_forward=False, max_cc=0, fwd_from_self=False, fwd_without_lead=False):
    """The sequential rule -> SimpleNamespace(disposition [n], deferred
    [positions], records [the output list], p / ri / v {g: row}, r {(slot, g):
    row}, stats {counter index: value}).  A row holds the fields the call
    writes and `src`."""
    disp, kinds, closed = [], [], set()
    for m in recs:
        g = m["group"] - st.group_offset
        if is_bad(st, m):
            d, k = BAD, 0
        elif g in closed:  # rule 4
            d, k = DEFERRED, 0
        else:
            d, k = step(st, m, no_forward, fwd_without_lead)
            if d in (ROUTED, STEPDOWN):
                closed.add(g)
        disp.append(d)
        kinds.append(k)
    return _finish(st, recs, disp, kinds, max_cc, fwd_from_self)


def is_closer(st, m):
    """The order-free form's predicate: it reads the record and the resident
    rows, never another record."""
    g = m["group"] - st.group_offset
    rterm = int(st.term[g])
    if m["term"] > rterm:
        return True
    return (int(st.state[g]) == ST_LEADER and m["type"] != READ_INDEX_RESP and
            m["term"] in (0, rterm))


def route_by_stop(st, recs, no_forward=False, max_cc=0):
    """The order-free form the kernels use: stop[g] = the minimum of the keys
    (position + 1) of the group's closers; deferred iff key > stop[g]."""
    stop = {}
    for i, m in enumerate(recs):
        if not is_bad(st, m) and is_closer(st, m):
            g = m["group"] - st.group_offset
            stop[g] = min(stop.get(g, 1 << 32), i + 1)
    disp, kinds = [], []
    for i, m in enumerate(recs):
        g = m["group"] - st.group_offset
        if is_bad(st, m):
            d, k = BAD, 0
        elif i + 1 > stop.get(g, 1 << 32):
            d, k = DEFERRED, 0
        else:
            d, k = step(st, m, no_forward)
            assert (d in (ROUTED, STEPDOWN)) == (i + 1 == stop.get(g))
        disp.append(d)
        kinds.append(k)
    return _finish(st, recs, disp, kinds, max_cc)


def run_to_end(st, recs, **kw):
    """The deferred list fed back until it is empty (the resident rows do not
    change: a host would run the steps in between) -> the passes' outputs."""
    passes, pos = [], list(range(len(recs)))
    while pos:
        out = route(st, [recs[i] for i in pos], **kw)
        passes.append(out)
        pos = [pos[i] for i in out.deferred]
    return passes
