"""qe_outbox restated in plain Python (include/etcd_quorum.h states the rules):
the send masks of one leader-side call -> the ordered list of message records
and the statistics.  Imports no torch.

`st` carries the resident rows under the names of qe_progress (num_groups,
group_offset, num_slots, stride, log_runs, committed, last_index, run_first,
run_term, run_count, next, peer, snap_index, first_index), `inp` the fields of
qe_outbox_in; a row that is not given is None.  Rows are flat sequences indexed
[s * stride + g] / [r * stride + g] / [g]."""
from types import SimpleNamespace

APP, SNAP, HEARTBEAT, BAD = 1, 2, 3, 255
PR_REPLICATE, PF_STATE = 1, 3
MAX_MSG_RUNS, MAX_LOG_RUNS = 4, 16
M64 = (1 << 64) - 1
PHI, SALT = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
STAT_GROUPS, STAT_ENTRIES, STAT_APP, STAT_SNAP, STAT_HEARTBEAT, STAT_BAD = 0, 2, 4, 5, 6, 8
STAT_VIOLATIONS, STAT_CHECKSUM = 14, 15
FIELDS = ("group", "to", "type", "term", "index", "log_term", "commit", "ctx")


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def state(**kw):
    d = dict(num_groups=0, group_offset=0, num_slots=1, stride=0, log_runs=1, committed=None,
             last_index=None, run_first=None, run_term=None, run_count=None, next=None,
             peer=None, snap_index=None, first_index=None)
    d.update(kw)
    return SimpleNamespace(**d)


def inputs(**kw):
    d = dict(sent=None, snap=None, hb_sent=None, index=None, next_before=None, term=None,
             snap_term=None, hb_commit=None, hb_ctx=None, max_entries=0)
    d.update(kw)
    return SimpleNamespace(**d)


def runs_of(st, g):
    nr = min(int(st.run_count[g]), st.log_runs)
    return [(int(st.run_first[r * st.stride + g]), int(st.run_term[r * st.stride + g]))
            for r in range(nr)]


def term_at(runs, li, i):
    """raftLog.term on the run table: 0 outside [run_first[0], last_index]."""
    if not runs or i < runs[0][0] or i > li:
        return 0
    t = 0
    for f, rt in runs:
        if i >= f:
            t = rt
    return t


def app_index(st, inp, g, s, replicate_before=True):
    """m.Index of the MsgApp to slot s: the index row, else Next - 1 -- from
    before the call where the peer replicates now (the optimistic send moved
    Next), the current one otherwise."""
    k = s * st.stride + g
    if inp.index is not None:
        return int(inp.index[k])
    repl = (int(st.peer[k]) & PF_STATE) == PR_REPLICATE
    row = inp.next_before if repl == replicate_before else st.next
    return (int(row[k]) - 1) & M64


def entry_runs(runs, li, i, max_entries, msg_runs):
    """(i, hi] cut into the table's runs, at most msg_runs of them."""
    lim = max_entries if max_entries else 0xFFFFFFFF
    hi = i + lim if li - i > lim else li
    out = []
    for r, (f, t) in enumerate(runs):
        end = runs[r + 1][0] - 1 if r + 1 < len(runs) else li
        lo, e = max(f, i + 1), min(end, hi)
        if i < hi and lo <= e:
            if len(out) == msg_runs:
                break
            out.append((e - lo + 1, t))
    return out


def record(st, inp, g, s, kind, msg_runs, replicate_before=True):
    rec = dict(group=st.group_offset + g, to=s, type=kind, term=int(inp.term[g]), index=0,
               log_term=0, commit=0, ctx=0, ents=[])
    if kind == SNAP:
        si = int(st.snap_index[g]) if st.snap_index is not None else int(st.first_index[g]) - 1
        rec["index"] = si & M64
        rec["log_term"] = (int(inp.snap_term[g]) if inp.snap_term is not None
                           else term_at(runs_of(st, g), int(st.last_index[g]), rec["index"]))
    elif kind == APP:
        runs, li = runs_of(st, g), int(st.last_index[g])
        i = rec["index"] = app_index(st, inp, g, s, replicate_before)
        if not runs or i < runs[0][0] or i > li:
            rec["type"] = BAD
        else:
            rec["log_term"] = term_at(runs, li, i)
            rec["commit"] = int(st.committed[g])
            rec["ents"] = entry_runs(runs, li, i, inp.max_entries, msg_runs)
    else:
        rec["commit"] = int(inp.hb_commit[s * st.stride + g])
        rec["ctx"] = int(inp.hb_ctx[g]) if inp.hb_ctx is not None else 0
    return rec


def build(st, inp, msg_runs=MAX_MSG_RUNS, replicate_before=True):
    """-> (records in list order, stats as {counter index: value}).
    replicate_before=False swaps the StateReplicate rule (a negative control)."""
    G, S = st.num_groups, st.num_slots
    full = (1 << S) - 1
    get = lambda row, g: 0 if row is None else int(row[g]) & full  # noqa: E731
    recs, groups = [], 0
    for t0 in range(0, G, 64):
        tile = range(t0, min(G, t0 + 64))
        masks = {g: (get(inp.sent, g), get(inp.snap, g), get(inp.hb_sent, g)) for g in tile}
        groups += sum(1 for m in masks.values() if any(m))
        for s in range(S):
            for g in tile:
                sent, snap, hb = (m >> s & 1 for m in masks[g])
                if snap:
                    recs.append(record(st, inp, g, s, SNAP, msg_runs))
                elif sent:
                    recs.append(record(st, inp, g, s, APP, msg_runs, replicate_before))
                elif hb:
                    recs.append(record(st, inp, g, s, HEARTBEAT, msg_runs))
    stats = {k: 0 for k in (STAT_GROUPS, STAT_ENTRIES, STAT_APP, STAT_SNAP, STAT_HEARTBEAT,
                            STAT_BAD, STAT_VIOLATIONS, STAT_CHECKSUM)}
    stats[STAT_GROUPS] = groups
    by_type = {APP: STAT_APP, SNAP: STAT_SNAP, HEARTBEAT: STAT_HEARTBEAT, BAD: STAT_BAD}
    for r in recs:
        ents = sum(n for n, _ in r["ents"])
        stats[by_type[r["type"]]] += 1
        stats[STAT_VIOLATIONS] += r["type"] == BAD
        stats[STAT_ENTRIES] += ents
        h = mix64((r["group"] * PHI) ^ SALT ^ (r["type"] << 56) ^ (r["to"] << 48))
        for x in (r["index"], r["log_term"], r["commit"], ents):
            h = mix64(h ^ x)
        stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
    return recs, stats


def truncate(recs, capacity):
    """What the arrays hold: the first min(count, capacity) records."""
    return len(recs), recs[:capacity]
