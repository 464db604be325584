"""CPU model of qe_follower_step: the reference's follower restated on an
explicit list of (index, term) entries, function by function as written --
raftLog.term / matchTerm / findConflict (the linear loop) / findConflictByTerm
(index by index) / maybeAppend / append / commitTo (raft/log.go:88-168,
:233-241, :265-285, :317-323), unstable.truncateAndAppend, the term preamble
of raft.Step (raft/raft.go:847-920), stepFollower / stepCandidate's MsgApp and
MsgHeartbeat arms, handleAppendEntries / handleHeartbeat (:1475-1516) and
becomeFollower / reset (:590-619, :686-693).  Nothing here is computed on
runs, so it shares no closed form with the kernel.

The run table is bookkeeping next to the entries: it is cut and extended by
the rule include/etcd_quorum.h states (runs starting at or after ci dropped,
a piece of another term than the last run's a new row), and after every step
the expanded table must equal the entry list.

Also here: the random generator of states and messages the CPU and the GPU
tests share, and the packing of a list of nodes into the arrays of the ABI.
"""
import copy

import numpy as np

from tests.tick_model import mix64 as mix64_np

M64 = (1 << 64) - 1
NONE_SLOT = 0xFF

ST_FOLLOWER, ST_CANDIDATE, ST_LEADER, ST_PRE_CANDIDATE = 0, 1, 2, 3
LMSG_NONE, LMSG_APP, LMSG_HEARTBEAT = 0, 1, 2
FOLLOW_CHECK_QUORUM, FOLLOW_PREVOTE = 1, 2
TEV_HEARD, TEV_RESET = 1, 2
MAX_MSG_RUNS = 4

FR_NONE, FR_IGNORED, FR_LOWER_TERM_RESP, FR_HEARTBEAT_RESP = 0, 1, 2, 3
FR_APP_ACCEPT, FR_APP_REJECT, FR_APP_STALE = 4, 5, 6
FR_REFUSED = 16
FR_BAD_MSG, FR_COMMIT_PAST_LOG, FR_CONFLICT_COMMITTED, FR_RUNS_FULL, FR_APP_GAP = 16, 17, 18, 19, 20
FR_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("FR_") and k != "FR_REFUSED"}

STAT_GROUPS, STAT_GRANTED, STAT_REJECTED, STAT_APPENDED = 0, 7, 8, 2
STAT_COMMIT_ADVANCED, STAT_VIOLATIONS, STAT_CHECKSUM = 9, 14, 15
PHI, FOLLOW_SALT = 0x9E3779B97F4A7C15, 0x2545F4914F6CDD1D


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Refused(Exception):
    """A panic of the reference (or input the ABI refuses): the step is undone."""

    def __init__(self, code):
        super().__init__(FR_NAMES[code])
        self.code = code


class Msg:
    def __init__(self, type=LMSG_NONE, frm=0, term=0, index=0, log_term=0, commit=0, runs=()):
        self.type, self.frm, self.term = int(type), int(frm), int(term)
        self.index, self.log_term, self.commit = int(index), int(log_term), int(commit)
        self.runs = [(int(n), int(t)) for n, t in runs]  # (ent_len, ent_term)

    def entries(self):
        out, i = [], self.index
        for n, t in self.runs:
            for _ in range(n):
                i += 1
                out.append((i, t))
        return out


def runs_of(ents):
    """The canonical run table of an entry list (ents[0] the dummy entry)."""
    runs = []
    for i, t in ents:
        if not runs or runs[-1][1] != t:
            runs.append((i, t))
    return runs


def expand(runs, last):
    """orc_log_term over [runs[0].first, last]."""
    out = []
    for i in range(runs[0][0], last + 1):
        t = runs[0][1]
        for f, rt in runs:
            if i >= f:
                t = rt
        out.append((i, t))
    return out


class Node:
    """One raft group as its receiver sees it: ents[0] is the dummy (snapshot)
    entry, ents[1:] the log."""

    def __init__(self, ents, committed=0, term=0, state=ST_FOLLOWER, lead=NONE_SLOT,
                 vote=NONE_SLOT, transferee=NONE_SLOT, runs=None):
        self.ents = [(int(i), int(t)) for i, t in ents]
        self.committed, self.term, self.state = int(committed), int(term), int(state)
        self.lead, self.vote, self.transferee = int(lead), int(vote), int(transferee)
        self.runs = list(runs) if runs is not None else runs_of(self.ents)
        self.check()

    def check(self):
        assert expand(self.runs, self.last_index()) == self.ents, (self.runs, self.ents)

    # ---- raftLog ----
    def last_index(self):
        return self.ents[-1][0]

    def log_term(self, i):  # log.go:265-285
        dummy = self.ents[0][0]
        if i < dummy or i > self.last_index():
            return 0
        return self.ents[i - dummy][1]

    def match_term(self, i, t):  # log.go:317-323
        return self.log_term(i) == t

    def find_conflict(self, ents):  # log.go:127-138
        for i, t in ents:
            if not self.match_term(i, t):
                return i
        return 0

    def find_conflict_by_term(self, index, t):  # log.go:147-168
        if index > self.last_index():
            return index
        while True:
            if self.log_term(index) <= t:
                break
            index = (index - 1) & M64
        return index

    def commit_to(self, tocommit):  # log.go:233-241
        if self.committed < tocommit:
            if self.last_index() < tocommit:
                raise Refused(FR_COMMIT_PAST_LOG)
            self.committed = tocommit

    def truncate_and_append(self, ents, log_runs):  # log_unstable.go truncateAndAppend
        after = ents[0][0] - 1
        last = self.last_index()
        if after > last:  # u.slice past the end: the slice-bounds panic
            raise Refused(FR_APP_GAP)
        dummy = self.ents[0][0]
        assert after >= dummy
        self.ents = self.ents[: after - dummy + 1] + list(ents)
        # the run table, by the ABI's rule
        ci = ents[0][0]
        runs = [r for r in self.runs if r[0] < ci]
        for i, t in ents:
            if runs[-1][1] != t:
                runs.append((i, t))
        if len(runs) > log_runs:
            raise Refused(FR_RUNS_FULL)
        self.runs = runs

    def append(self, ents, log_runs):  # log.go:106-115
        if not ents:
            return self.last_index()
        if ents[0][0] - 1 < self.committed:
            raise Refused(FR_CONFLICT_COMMITTED)
        self.truncate_and_append(ents, log_runs)
        return self.last_index()

    def maybe_append(self, index, log_term, committed, ents, log_runs):  # log.go:88-104
        """-> (lastnewi, ok, ci)"""
        if self.match_term(index, log_term):
            lastnewi = index + len(ents)
            ci = self.find_conflict(ents)
            if ci == 0:
                pass
            elif ci <= self.committed:
                raise Refused(FR_CONFLICT_COMMITTED)
            else:
                self.append(ents[ci - (index + 1):], log_runs)
            self.commit_to(min(committed, lastnewi))
            return lastnewi, True, ci
        return 0, False, 0

    # ---- raft ----
    def become_follower(self, term, lead):  # raft.go:686-693, reset :590-619
        if self.term != term:
            self.term = term
            self.vote = NONE_SLOT
        self.lead = NONE_SLOT
        self.transferee = NONE_SLOT  # abortLeaderTransfer
        self.lead = lead
        self.state = ST_FOLLOWER

    def handle_append_entries(self, m, log_runs, out):  # raft.go:1475-1511
        if m.index < self.committed:
            out.update(result=FR_APP_STALE, resp_index=self.committed)
            return
        lastnewi, ok, ci = self.maybe_append(m.index, m.log_term, m.commit, m.entries(), log_runs)
        if ok:
            out.update(result=FR_APP_ACCEPT, resp_index=lastnewi, append_from=ci)
            if ci:
                out["appended"] = lastnewi - ci + 1
        else:
            hint = self.find_conflict_by_term(min(m.index, self.last_index()), m.log_term)
            out.update(result=FR_APP_REJECT, resp_index=m.index, reject_hint=hint,
                       resp_log_term=self.log_term(hint))

    def handle_heartbeat(self, m, out):  # raft.go:1513-1516
        self.commit_to(m.commit)
        out.update(result=FR_HEARTBEAT_RESP)


def bad_msg(m, num_slots):
    if m.type not in (LMSG_APP, LMSG_HEARTBEAT) or m.frm >= num_slots:
        return True
    if m.type == LMSG_APP:
        prev = n = 0
        for ln, t in m.runs:
            if ln:
                if t == 0 or t < prev:
                    return True
                prev = t
            n += ln
        if m.index + n >= M64:  # wrapping, or reaching 2^64 - 1: no log index
            return True
    return False


def step(node, m, flags=0, num_slots=16, log_runs=16):
    """raft.Step for one MsgApp / MsgHeartbeat.  Returns (node after, out):
    `out` holds `result` and exactly the output fields the call writes for the
    group (events always); `appended` is the statistic's share."""
    out = {"result": FR_NONE, "events": 0}
    if m.type == LMSG_NONE:
        return node, out
    if bad_msg(m, num_slots):
        out["result"] = FR_BAD_MSG
        return node, out
    blank = {"resp_index": 0, "append_from": 0}
    if m.term < node.term:  # raft.go:883-919
        out.update(blank)
        out["result"] = FR_LOWER_TERM_RESP if flags & 3 else FR_IGNORED
        return node, out
    n = copy.deepcopy(node)
    if m.term > n.term:  # :876-877
        n.become_follower(m.term, m.frm)
        out["events"] = TEV_RESET
    elif n.state == ST_LEADER:  # stepLeader: no arm for MsgApp / MsgHeartbeat
        out.update(blank)
        out["result"] = FR_IGNORED
        return node, out
    elif n.state in (ST_CANDIDATE, ST_PRE_CANDIDATE):  # stepCandidate :1390-1395
        n.become_follower(m.term, m.frm)
        out["events"] = TEV_RESET
    else:  # stepFollower :1433-1440
        n.lead = m.frm
        out["events"] = TEV_HEARD
    out.update(blank)
    try:
        if m.type == LMSG_APP:
            n.handle_append_entries(m, log_runs, out)
        else:
            n.handle_heartbeat(m, out)
    except Refused as e:
        return node, {"result": e.code, "events": 0}
    n.check()
    return n, out


def group_stats(gid, before, after, out):
    """The share of one group with a message in the statistics vector."""
    s = {STAT_GROUPS: 1}
    r = out["result"]
    s[STAT_GRANTED] = int(r == FR_APP_ACCEPT)
    s[STAT_REJECTED] = int(r == FR_APP_REJECT)
    s[STAT_APPENDED] = out.get("appended", 0)
    s[STAT_COMMIT_ADVANCED] = int(after.committed > before.committed)
    s[STAT_VIOLATIONS] = int(r >= FR_REFUSED)
    h = mix64(((gid * PHI) & M64) ^ FOLLOW_SALT ^ (r << 56))
    h = mix64(h ^ after.term)
    h = mix64(h ^ after.committed)
    h = mix64(h ^ after.last_index())
    s[STAT_CHECKSUM] = h
    return s


def hash_chain(gid, salt, result, words):
    """The checksum term of group_stats over arrays of groups (uint64,
    wrapping): mix64 of the group id, the salt and the result, then one mix64
    per state word."""
    u64 = lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        h = mix64_np((u64(gid) * np.uint64(PHI)) ^ np.uint64(salt) ^ (u64(result) << np.uint64(56)))
        for w in words:
            h = mix64_np(h ^ u64(w))
    return h


def group_hashes(gid, result, term, committed, last_index):
    """group_stats' STAT_CHECKSUM, vectorised (the state words are the ones after the step)."""
    return hash_chain(gid, FOLLOW_SALT, result, (term, committed, last_index))


# ---------------------------------------------------------------------------
# The random generator (shared by tests/test_follower_model.py and
# tests/test_gpu_follower.py).
# ---------------------------------------------------------------------------
def gen_node(rng, R, S):
    dummy = int(rng.integers(0, 6))
    t = int(rng.integers(0, 3)) if dummy else 0
    k = int(rng.integers(1, R + 1))
    runs, ents, i = [], [], dummy
    for r in range(k):
        if r:
            # mostly a higher term; sometimes the same one (a table that is
            # not canonical is still a valid table)
            t += int(rng.integers(0 if rng.random() < 0.05 else 1, 3))
        runs.append((i, t))
        for _ in range(int(rng.integers(1, 4))):
            ents.append((i, t))
            i += 1
    last = ents[-1][0]
    state = int(rng.choice([ST_FOLLOWER] * 7 + [ST_CANDIDATE, ST_LEADER, ST_PRE_CANDIDATE]))
    slot = lambda: int(rng.integers(0, S)) if rng.random() < 0.7 else NONE_SLOT  # noqa: E731
    return Node(ents, committed=int(rng.integers(dummy, last + 1)),
                term=ents[-1][1] + int(rng.integers(0, 3)), state=state, lead=slot(),
                vote=slot(), transferee=slot(), runs=runs)


def _to_runs(terms, E, rng):
    """Term runs of a list of entry terms, at most E of them (the list is cut
    short where it would need more), with an empty run put in now and then."""
    runs = []
    for t in terms:
        if runs and runs[-1][1] == t:
            runs[-1][0] += 1
        elif len(runs) < E:
            runs.append([1, t])
        else:
            break
    if len(runs) < E and rng.random() < 0.3:
        pos = int(rng.integers(0, len(runs) + 1))
        t = runs[pos - 1][1] if pos else (runs[0][1] if runs else int(rng.integers(0, 4)))
        runs.insert(pos, [0, t if rng.random() < 0.7 or pos else 0])
    return [tuple(r) for r in runs]


def gen_msg(rng, node, E, S):
    u = rng.random()
    if u < 0.10:
        return Msg()
    m = Msg(type=LMSG_APP if u < 0.72 else LMSG_HEARTBEAT, frm=int(rng.integers(0, S)))
    if rng.random() < 0.02:
        m.type = int(rng.integers(3, 256))
    if rng.random() < 0.02:
        m.frm = int(rng.integers(S, 256))
    v = rng.random()
    m.term = node.term
    if v < 0.12:
        m.term = node.term + int(rng.integers(1, 4))
    elif v < 0.22 and node.term:
        m.term = node.term - int(rng.integers(1, node.term + 1))
    last, dummy = node.last_index(), node.ents[0][0]
    m.commit = int(rng.integers(0, last + 1))
    if rng.random() < 0.04:
        m.commit = last + int(rng.integers(1, 4))
    if m.type != LMSG_APP:
        return m
    k = rng.random()
    top = max(m.term, node.ents[-1][1])
    if k < 0.40:  # an append at the tail
        m.index, m.log_term = last, node.log_term(last)
        t, terms = node.ents[-1][1], []
        for _ in range(int(rng.integers(0, 7))):
            t += int(rng.random() < 0.35) * int(rng.integers(1, 3))
            terms.append(t)
        m.runs = _to_runs(terms, E, rng)
    elif k < 0.72:  # entries that overlap the log, agreeing up to some point
        m.index = int(rng.integers(node.committed, last + 1))
        m.log_term = node.log_term(m.index)
        nent = int(rng.integers(0, 8))
        split = int(rng.integers(0, nent + 1)) if rng.random() < 0.7 else nent
        terms, t = [], None
        for j in range(nent):
            i = m.index + 1 + j
            if j < split and i <= last:
                t = node.log_term(i)
            else:
                base = t if t is not None else node.log_term(min(i, last))
                t = base + (int(rng.integers(1, 3)) if j == split or rng.random() < 0.3 else 0)
                t = max(t, 1)
            terms.append(t)
        m.runs = _to_runs(terms, E, rng)
    elif k < 0.88:  # a probe that does not match
        m.index = int(rng.integers(dummy, last + 4))
        m.log_term = max(0, node.log_term(min(m.index, last)) + int(rng.integers(-2, 3)))
        m.runs = _to_runs([top + 1] * int(rng.integers(0, 3)), E, rng)
    elif k < 0.94:  # below the commit
        m.index = int(rng.integers(0, node.committed + 1))
        m.log_term = node.log_term(m.index)
        m.runs = _to_runs([top] * int(rng.integers(0, 3)), E, rng)
    elif k < 0.97:  # past the log with LogTerm 0, which term() "matches"
        m.index, m.log_term = last + int(rng.integers(1, 4)), 0
        m.runs = _to_runs([top] * int(rng.integers(0, 3)), E, rng)
    else:  # malformed runs
        m.index, m.log_term = last, node.log_term(last)
        m.runs = [(2, top + 2), (1, top + 1)][:E] if rng.random() < 0.5 else [(1, 0)][:E]
        if rng.random() < 0.3:
            m.index = M64 - int(rng.integers(0, 2))
            m.runs = [(3, top + 1)][:E]
    return m


# ---------------------------------------------------------------------------
# Nodes and messages as the arrays of the ABI.
# ---------------------------------------------------------------------------
def pack_nodes(nodes, R, stride, fill=0):
    G = len(nodes)
    a = {
        "committed": np.array([n.committed for n in nodes], np.uint64),
        "last_index": np.array([n.last_index() for n in nodes], np.uint64),
        "run_count": np.array([len(n.runs) for n in nodes], np.uint8),
        "run_first": np.full(R * stride, fill, np.uint64),
        "run_term": np.full(R * stride, fill, np.uint64),
        "term": np.array([n.term for n in nodes], np.uint64),
        "state": np.array([n.state for n in nodes], np.uint8),
        "lead": np.array([n.lead for n in nodes], np.uint8),
        "vote": np.array([n.vote for n in nodes], np.uint8),
        "lead_transferee": np.array([n.transferee for n in nodes], np.uint8),
    }
    for g, n in enumerate(nodes):
        assert len(n.runs) <= R
        for r, (f, t) in enumerate(n.runs):
            a["run_first"][r * stride + g] = f
            a["run_term"][r * stride + g] = t
    assert G <= stride
    return a


def pack_msgs(msgs, E, stride):
    a = {
        "type": np.array([m.type for m in msgs], np.uint8),
        "from": np.array([m.frm for m in msgs], np.uint8),
        "term": np.array([m.term for m in msgs], np.uint64),
        "index": np.array([m.index for m in msgs], np.uint64),
        "log_term": np.array([m.log_term for m in msgs], np.uint64),
        "commit": np.array([m.commit for m in msgs], np.uint64),
        "ent_len": np.zeros(max(E, 1) * stride, np.uint32),
        "ent_term": np.zeros(max(E, 1) * stride, np.uint64),
    }
    for g, m in enumerate(msgs):
        assert len(m.runs) <= E
        for j, (n, t) in enumerate(m.runs):
            a["ent_len"][j * stride + g] = n
            a["ent_term"][j * stride + g] = t
    return a


def step_batch(nodes, msgs, flags, num_slots, log_runs, group_offset=0):
    """-> (nodes after, outs, stats dict)"""
    after, outs, stats = [], [], {}
    for g, (n, m) in enumerate(zip(nodes, msgs)):
        n2, o = step(n, m, flags, num_slots, log_runs)
        after.append(n2)
        outs.append(o)
        if m.type != LMSG_NONE:
            for k, v in group_stats(group_offset + g, n, n2, o).items():
                stats[k] = (stats.get(k, 0) + v) & M64
    return after, outs, stats
