"""qe_inbox restated in plain Python (include/etcd_quorum.h states the rules):
a list of delivered messages in delivery order -> the message rows of
qe_follower_step, qe_snapshot_step, qe_progress_step and qe_vote_step for one
pass of calls, a disposition per record, the deferred list and the statistics.
This is the SEQUENTIAL rule, a restatement of tests/cluster_sim.py Sim.deliver;
the kernels compute it in an order-free form.  With it duties H4 and H6 of a
host and the QE_TICK_HUP half of H1 are optional.  Imports no torch.

A record is a dict: group (the receiver's global id), from, type (IMSG_*),
term, index, log_term, commit, hint, ctx, flags, ents [(len, term), ...].  `st`
carries num_groups, group_offset, num_slots, stride and the rows term[G] and
state[G] of qe_follower."""
from types import SimpleNamespace

import numpy as np

from tests.tick_model import mix64 as mix64_np

APP, SNAP, HEARTBEAT = 1, 2, 3
APP_RESP, APP_RESP_REJECT, HEARTBEAT_RESP, SNAP_STATUS, SNAP_STATUS_REJECT = 4, 5, 6, 7, 8
UNREACHABLE, TRANSFER_LEADER = 9, 10
VOTE, PREVOTE, VOTE_RESP, PREVOTE_RESP, TIMEOUT_NOW, HUP = 11, 12, 13, 14, 15, 16
F_CLS, S_CLS, R_CLS, V_CLS = "F", "S", "R", "V"
ROUTED, STEPDOWN, DEFERRED, DROP_LOWER_TERM, DROP_NOT_LEADER, BAD = 1, 2, 3, 4, 5, 255
ID_NAMES = {1: "ROUTED", 2: "STEPDOWN", 3: "DEFERRED", 4: "DROP_LOWER_TERM",
            5: "DROP_NOT_LEADER", 255: "BAD"}
SRC_TICK = 0xFFFFFFFF
TICK_HUP = 1
ST_LEADER = 2
LMSG_APP, LMSG_HEARTBEAT, SMSG_SNAP = 1, 2, 1
VMSG = {VOTE: 1, PREVOTE: 2, VOTE_RESP: 3, PREVOTE_RESP: 4, HUP: 5, TIMEOUT_NOW: 6}
VMSG_VOTE_RESP, VMSG_HUP, VMF_REJECT = 3, 5, 2
M64 = (1 << 64) - 1
PHI, SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
STAT_GROUPS, STAT_BAD, STAT_ROUTED, STAT_LOWER_TERM, STAT_DEFERRED = 0, 1, 4, 5, 6
STAT_NOT_LEADER, STAT_STEPDOWN, STAT_VIOLATIONS, STAT_CHECKSUM = 8, 13, 14, 15
BY_DISPOSITION = {ROUTED: STAT_ROUTED, STEPDOWN: STAT_STEPDOWN, DEFERRED: STAT_DEFERRED,
                  DROP_LOWER_TERM: STAT_LOWER_TERM, DROP_NOT_LEADER: STAT_NOT_LEADER,
                  BAD: STAT_BAD}


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def record_hash(group, disp, type, frm, i):
    """The STAT_CHECKSUM term of record i of the list."""
    h = mix64((group * PHI) ^ SALT ^ (disp << 56) ^ (type << 48) ^ (frm << 40))
    return mix64(h ^ i)


def record_hashes(group, disp, type, frm, salt=SALT):
    """record_hash over the arrays of a whole list (position = array index),
    vectorised -> uint64[n]; tests/test_inbox_model.py pins it to the scalar
    form.  `salt`: tests/requests_model.py hashes the same words under its own."""
    u =lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        h = mix64_np((u(group) * np.uint64(PHI)) ^ np.uint64(salt) ^ (u(disp) << np.uint64(56)) ^
                     (u(type) << np.uint64(48)) ^ (u(frm) << np.uint64(40)))
    return mix64_np(h ^ np.arange(len(h), dtype=np.uint64))


def cls_of(t):
    if t in (APP, HEARTBEAT):
        return F_CLS
    if t == SNAP:
        return S_CLS
    if APP_RESP <= t <= TRANSFER_LEADER:
        return R_CLS
    if VOTE <= t <= HUP:
        return V_CLS
    return None


def rec(group, frm, type, term=0, index=0, log_term=0, commit=0, hint=0, ctx=0, flags=0, ents=()):
    return {"group": int(group), "from": int(frm), "type": int(type), "term": int(term),
            "index": int(index), "log_term": int(log_term), "commit": int(commit),
            "hint": int(hint), "ctx": int(ctx), "flags": int(flags),
            "ents": [(int(n), int(t)) for n, t in ents]}


def state(**kw):
    d = dict(num_groups=0, group_offset=0, num_slots=1, stride=0, term=None, state=None)
    d.update(kw)
    return SimpleNamespace(**d)


def route(st, recs, tick_action=None, msg_runs=4, same_from_joins=False):
    """-> SimpleNamespace(disposition [n], deferred [positions], f / s / v
    {g: row}, r {(slot, g): row}, stats {counter index: value}, waves {g:
    [positions]}).  A row holds the fields the call writes and `src`.
    same_from_joins=True lets a response of a slot the wave already holds join
    it (a negative control)."""
    G, S, goff = st.num_groups, st.num_slots, st.group_offset
    n = len(recs)
    disp = [None] * n
    waves, closed, froms = {}, set(), {}
    out = SimpleNamespace(f={}, s={}, v={}, r={}, waves=waves)
    # ---- the virtual HUP of a tick opens its group's wave before position 0 ----
    for g in range(G):
        if tick_action is not None and int(tick_action[g]) & TICK_HUP:
            waves[g] = [SRC_TICK]
            out.v[g] = dict(type=VMSG_HUP, frm=0, term=0, index=0, log_term=0, flags=0,
                            src=SRC_TICK)
    # ---- wave forming ----
    for i, m in enumerate(recs):
        g, c = m["group"] - goff, cls_of(m["type"])
        if not 0 <= g < G or c is None or (m["from"] >= S and m["type"] != HUP):
            disp[i] = BAD
            continue
        opener = waves.get(g)
        if opener is None:
            waves[g], froms[g] = [i], {m["from"]}
        elif (g not in closed and opener[0] != SRC_TICK and c == R_CLS and
              cls_of(recs[opener[0]]["type"]) == R_CLS and
              (same_from_joins or m["from"] not in froms[g])):
            waves[g].append(i)
            froms[g].add(m["from"])
        else:
            closed.add(g)
            disp[i] = DEFERRED
    # ---- routing ----
    for g, members in waves.items():
        if members[0] == SRC_TICK:
            continue
        m = recs[members[0]]
        c = cls_of(m["type"])
        if c == F_CLS:
            app = m["type"] == APP
            ents = (list(m["ents"][:msg_runs]) + [(0, 0)] * msg_runs)[:msg_runs] if app else None
            out.f[g] = dict(type=LMSG_APP if app else LMSG_HEARTBEAT, frm=m["from"],
                            term=m["term"], index=m["index"], log_term=m["log_term"],
                            commit=m["commit"], ents=ents, src=members[0])
        elif c == S_CLS:
            out.s[g] = dict(type=SMSG_SNAP, frm=m["from"], term=m["term"], snap_index=m["index"],
                            snap_term=m["log_term"], src=members[0])
        elif c == V_CLS:
            out.v[g] = dict(type=VMSG[m["type"]], frm=m["from"], term=m["term"],
                            index=m["index"], log_term=m["log_term"], flags=m["flags"],
                            src=members[0])
        if c != R_CLS:
            disp[members[0]] = ROUTED
            continue
        rterm, leads = int(st.term[g]), int(st.state[g]) == ST_LEADER
        for i in members:  # Step's preamble, in list order
            m = recs[i]
            if m["term"] != 0 and m["term"] < rterm:
                disp[i] = DROP_LOWER_TERM
            elif m["term"] != 0 and m["term"] > rterm:
                if g in out.v:
                    disp[i] = DEFERRED
                else:
                    disp[i] = STEPDOWN
                    out.v[g] = dict(type=VMSG_VOTE_RESP, frm=m["from"], term=m["term"], index=0,
                                    log_term=0, flags=VMF_REJECT, src=i)
            elif not leads:
                disp[i] = DROP_NOT_LEADER
            else:
                disp[i] = ROUTED
                out.r[(m["from"], g)] = dict(type=m["type"] - 3, index=m["index"], hint=m["hint"],
                                             log_term=m["log_term"], ctx=m["ctx"], src=i)
    out.disposition = disp
    out.deferred = [i for i in range(n) if disp[i] == DEFERRED]
    # ---- the statistics ----
    stats = {k: 0 for k in list(BY_DISPOSITION.values()) + [STAT_GROUPS, STAT_VIOLATIONS,
                                                            STAT_CHECKSUM]}
    stats[STAT_GROUPS] = len({recs[i]["group"] for i in range(n) if disp[i] == ROUTED})
    for i, m in enumerate(recs):
        stats[BY_DISPOSITION[disp[i]]] += 1
        stats[STAT_VIOLATIONS] += disp[i] == BAD
        h = record_hash(m["group"], disp[i], m["type"], m["from"], i)
        stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
    out.stats = stats
    return out
