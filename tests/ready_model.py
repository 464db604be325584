"""qe_ready_note, qe_ready and qe_advance restated sequentially in plain
Python (include/etcd_quorum.h states the rules).  Imports no torch.

`st` carries the resident rows under the names of qe_progress and qe_follower
(num_groups, group_offset, num_slots, stride, log_runs, committed, last_index,
run_first, run_term, run_count; term, state, lead, vote -- vote may be None),
`rs` the eight rows of qe_ready_state.  Rows are flat sequences indexed
[r * stride + g] / [g]; the three functions write into the rows of `rs` in
place (numpy arrays or lists).  A record is a dict of the fields of
qe_ready_out, with `ents` / `apply` the listed term runs as (len, term)."""
from types import SimpleNamespace

from tests.outbox_model import M64, PHI, mix64, runs_of, term_at

FR_APP_ACCEPT, SR_RESTORED, ST_LEADER = 4, 5, 2
SOFT, HARD, MUST_SYNC, SNAP, ENTS_CUT, APPLY_CUT = 1, 2, 4, 8, 16, 32
ADV_OK, ADV_OK_STALE_ENTRIES, ADV_BAD_GROUP, ADV_APPLIED_RANGE, ADV_AUTO_LEAVE = 1, 2, 8, 9, 0x10
NONE = 0xFF
SALT = 0x8CB92BA72F3D8DD7
STAT_GROUPS, STAT_ENTRIES, STAT_MUST_SYNC, STAT_APPLY, STAT_CHECKSUM = 0, 2, 4, 9, 15
STATE_ROWS = ("stable", "applied", "snap_pending", "prev_term", "prev_commit", "prev_vote",
              "prev_lead", "prev_state")
FIELDS = ("group", "term", "commit", "vote", "lead", "state", "flags", "ent_first", "ent_count",
          "ent_last_term", "apply_first", "apply_count", "snap_index")


def state(**kw):
    d = dict(num_groups=0, group_offset=0, num_slots=1, stride=0, log_runs=1, committed=None,
             last_index=None, run_first=None, run_term=None, run_count=None, term=None,
             state=None, lead=None, vote=None)
    d.update(kw)
    return SimpleNamespace(**d)


def ready_state(**kw):
    return SimpleNamespace(**kw)


def reset(st, rs):
    """NewRawNode: prev := current, stable = last_index, snap_pending = 0."""
    for g in range(st.num_groups):
        rs.stable[g], rs.snap_pending[g] = st.last_index[g], 0
        rs.prev_term[g], rs.prev_commit[g] = st.term[g], st.committed[g]
        rs.prev_vote[g] = NONE if st.vote is None else st.vote[g]
        rs.prev_lead[g], rs.prev_state[g] = st.lead[g], st.state[g]


def slot(v, S):
    return int(v) if int(v) < S else NONE


def note(st, rs, follow_result=None, append_from=None, snap_result=None, snap_resp_index=None):
    """unstable.truncateAndAppend's `after <= offset` arm, then unstable.restore."""
    for g in range(st.num_groups):
        if follow_result is not None and int(follow_result[g]) == FR_APP_ACCEPT:
            af = int(append_from[g])
            if af != 0 and af - 1 < int(rs.stable[g]):
                rs.stable[g] = af - 1
        if snap_result is not None and int(snap_result[g]) == SR_RESTORED:
            rs.stable[g] = rs.snap_pending[g] = int(snap_resp_index[g])


def cut(runs, li, i, hi, ent_runs):
    """(i, hi] cut into the table's runs, at most ent_runs of them (qe_outbox
    rule 4, its cap of 0xFFFFFFFF entries included) -> [(len, term), ...]."""
    out = []
    hi = min(hi, i + 0xFFFFFFFF)
    for r, (f, t) in enumerate(runs):
        end = runs[r + 1][0] - 1 if r + 1 < len(runs) else li
        lo, e = max(f, i + 1), min(end, hi)
        if i < hi and lo <= e:
            if len(out) == ent_runs:
                break
            out.append((e - lo + 1, t))
    return out


def group_ready(st, rs, g, pending=0, max_apply=0, ent_runs=0, sync_from_commit=False):
    """-> the record of group g, or None where it is not listed."""
    S = st.num_slots
    term, commit, li = int(st.term[g]), int(st.committed[g]), int(st.last_index[g])
    vote = NONE if st.vote is None else slot(st.vote[g], S)
    lead, state_ = slot(st.lead[g], S), int(st.state[g])
    pterm, pcommit = int(rs.prev_term[g]), int(rs.prev_commit[g])
    pvote, plead, pstate = slot(rs.prev_vote[g], S), slot(rs.prev_lead[g], S), int(rs.prev_state[g])
    stable, applied, snapp = int(rs.stable[g]), int(rs.applied[g]), int(rs.snap_pending[g])
    runs = runs_of(st, g)
    rf0 = int(st.run_first[g])
    hard_changed = (term, vote, commit) != (pterm, pvote, pcommit)
    hard_empty = (term, vote, commit) == (0, NONE, 0)
    soft = (lead, state_) != (plead, pstate)
    hard = hard_changed and not hard_empty
    has_ents = li > stable
    off = max((applied + 1) & M64, (rf0 + 1) & M64)
    has_apply = ((commit + 1) & M64) > off
    if not (soft or hard or snapp or has_ents or has_apply or pending):
        return None
    rec = dict(group=st.group_offset + g, term=term, commit=commit, vote=vote, lead=lead,
               state=state_, ent_first=(stable + 1) & M64, ent_count=0, ent_last_term=0,
               apply_first=0, apply_count=0, snap_index=snapp, ents=[], apply=[])
    flags = (SOFT if soft else 0) | (HARD if hard else 0) | (SNAP if snapp else 0)
    if has_ents:
        if ent_runs:
            rec["ents"] = cut(runs, li, stable, li, ent_runs)
            rec["ent_count"] = sum(n for n, _ in rec["ents"])
            rec["ent_last_term"] = rec["ents"][-1][1] if rec["ents"] else 0
        else:
            rec["ent_count"], rec["ent_last_term"] = li - stable, term_at(runs, li, li)
        if stable + rec["ent_count"] < li:
            flags |= ENTS_CUT
    if has_apply:
        want = commit + 1 - off
        hi = off + max_apply - 1 if max_apply and want > max_apply else commit
        if ent_runs:
            rec["apply"] = cut(runs, li, off - 1, hi, ent_runs)
            rec["apply_count"] = sum(n for n, _ in rec["apply"])
        else:
            rec["apply_count"] = hi + 1 - off
        rec["apply_first"] = off if rec["apply_count"] else 0
        if off + rec["apply_count"] - 1 < commit:
            flags |= APPLY_CUT
    sync = has_ents or vote != pvote or term != pterm
    if sync_from_commit:  # a negative control: MustSync from the whole HardState
        sync = has_ents or hard_changed
    rec["flags"] = flags | (MUST_SYNC if sync else 0)
    return rec


def ready(st, rs, pending=None, max_apply=0, ent_runs=0, **kw):
    """-> (records by ascending g, stats as {counter index: value})."""
    recs = []
    for g in range(st.num_groups):
        r = group_ready(st, rs, g, 0 if pending is None else int(pending[g]), max_apply, ent_runs,
                        **kw)
        if r is not None:
            recs.append(r)
    stats = {STAT_GROUPS: len(recs), STAT_ENTRIES: 0, STAT_MUST_SYNC: 0, STAT_APPLY: 0,
             STAT_CHECKSUM: 0}
    for r in recs:
        stats[STAT_ENTRIES] += r["ent_count"]
        stats[STAT_APPLY] += r["apply_count"]
        stats[STAT_MUST_SYNC] += bool(r["flags"] & MUST_SYNC)
        h = mix64((r["group"] * PHI) ^ SALT ^ (r["flags"] << 56) ^ (r["vote"] << 48) ^
                  (r["lead"] << 40) ^ (r["state"] << 32))
        for k in ("term", "commit", "ent_first", "ent_count", "ent_last_term", "apply_first",
                  "apply_count", "snap_index"):
            h = mix64(h ^ r[k])
        stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
    return recs, stats


def advance(st, rs, recs, auto_leave=None, pending_conf_index=None, move_stable=True):
    """acceptReady + RawNode.Advance + raft.advance -> one result per record.
    move_stable=False leaves `stable` alone (a negative control)."""
    out = []
    for r in recs:
        g = (r["group"] - st.group_offset) & M64
        if g >= st.num_groups:
            out.append(ADV_BAD_GROUP)
            continue
        na = ((r["apply_first"] + r["apply_count"] - 1) & M64 if r["apply_count"] else
              r["snap_index"] if r["flags"] & SNAP else 0)
        old = int(rs.applied[g])
        if na > 0 and (int(st.committed[g]) < na or na < old):
            out.append(ADV_APPLIED_RANGE)
            continue
        res = ADV_OK
        if na > 0:
            rs.applied[g] = na
        if r["flags"] & HARD:
            rs.prev_term[g], rs.prev_commit[g], rs.prev_vote[g] = r["term"], r["commit"], r["vote"]
        if r["flags"] & SOFT:
            rs.prev_lead[g], rs.prev_state[g] = r["lead"], r["state"]
        if r["ent_count"]:
            i, li = (r["ent_first"] + r["ent_count"] - 1) & M64, int(st.last_index[g])
            if int(rs.stable[g]) < i <= li and term_at(runs_of(st, g), li, i) == r["ent_last_term"]:
                if move_stable:
                    rs.stable[g] = i
            else:
                res = ADV_OK_STALE_ENTRIES
        if r["flags"] & SNAP and int(rs.snap_pending[g]) == r["snap_index"]:
            rs.snap_pending[g] = 0
        if (na > 0 and auto_leave is not None and int(auto_leave[g]) and
                int(st.state[g]) == ST_LEADER and old <= int(pending_conf_index[g]) <= na):
            res |= ADV_AUTO_LEAVE
        out.append(res)
    return out


def expand(first, runs):
    """The (term, index) list the term runs from `first` on stand for."""
    out, i = [], first
    for n, t in runs:
        for _ in range(n):
            out.append([t, i])
            i += 1
    return out
