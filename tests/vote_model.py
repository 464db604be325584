"""CPU model of qe_vote_step: the reference's election path restated function
by function on tests/follower_model.Node -- the term preamble of raft.Step
with the lease (raft/raft.go:849-920), the vote decision (:930-978),
stepCandidate's response arm with poll / RecordVote / TallyVotes (:1399-1414,
tracker.go:256-288, quorum/majority.go:178-210, joint.go:61-75), hup / campaign
(:760-835), MsgTimeoutNow (:1452-1457) and reset / becomeFollower /
becomeCandidate / becomePreCandidate / becomeLeader (:590-619, :686-759).  It
runs sequentially and mutates a copy, as the reference does: nothing is
shared with the kernel's branch-free form.

Node extends the follower model's node with the Votes map (voted / granted
bit masks), electionElapsed, the configuration masks (None = the array is
absent), the node's own slot and no_campaign.

Also here: the random generator of states and messages the CPU and the GPU
tests share, and the packing of a list of nodes into the arrays of the ABI.
"""
import copy

import numpy as np

from tests import follower_model as fm
from tests.follower_model import (M64, NONE_SLOT, ST_CANDIDATE, ST_FOLLOWER,  # noqa: F401
                                  ST_LEADER, ST_PRE_CANDIDATE, TEV_HEARD, TEV_RESET, mix64)

VMSG_NONE, VMSG_VOTE, VMSG_PREVOTE, VMSG_VOTE_RESP, VMSG_PREVOTE_RESP = 0, 1, 2, 3, 4
VMSG_HUP, VMSG_TIMEOUT_NOW = 5, 6
VMF_FORCE, VMF_REJECT = 1, 2
VOTE_CHECK_QUORUM, VOTE_PREVOTE = 1, 2
VR_NONE, VR_IGNORED, VR_IN_LEASE, VR_GRANT, VR_REJECT, VR_STEPPED_DOWN = 0, 1, 2, 3, 4, 5
VR_PENDING, VR_LOST, VR_CAMPAIGN_PREVOTE, VR_CAMPAIGN_VOTE, VR_WON = 6, 7, 8, 9, 10
VR_REFUSED = 16
VR_BAD_MSG = 16
VR_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("VR_") and k != "VR_REFUSED"}
ALL_RESULTS = set(VR_NAMES)

STAT_GROUPS, STAT_VOTE_PENDING, STAT_GRANTED, STAT_REJECTED = 0, 6, 7, 8
STAT_ELECTIONS, STAT_LEADERS, STAT_STEPDOWNS, STAT_VIOLATIONS, STAT_CHECKSUM = 11, 12, 13, 14, 15
PHI, VOTE_SALT = 0x9E3779B97F4A7C15, 0x9FB21C651E98DF25
VOTE_PENDING, VOTE_LOST, VOTE_WON = 1, 2, 3

CAMPAIGN_PRE_ELECTION, CAMPAIGN_ELECTION, CAMPAIGN_TRANSFER = "pre", "election", "transfer"


class Node(fm.Node):
    def __init__(self, ents, voted=0, granted=0, elapsed=0, inc=None, out=None, tracked=None,
                 self_slot=NONE_SLOT, no_campaign=0, **kw):
        super().__init__(ents, **kw)
        self.voted, self.granted, self.elapsed = int(voted), int(granted), int(elapsed)
        self.inc, self.out, self.tracked = inc, out, tracked
        self.self_slot, self.no_campaign = int(self_slot), int(no_campaign)
        # the invariant that makes lastTerm the last run row's term
        assert self.runs[-1][0] <= self.last_index(), (self.runs, self.last_index())

    def last_term(self):
        return self.log_term(self.last_index())

    def key(self):
        return (self.term, self.state, self.lead, self.vote, self.transferee, self.voted,
                self.granted)


class Msg:
    def __init__(self, type=VMSG_NONE, frm=0, term=0, index=0, log_term=0, flags=0):
        self.type, self.frm, self.term = int(type), int(frm), int(term)
        self.index, self.log_term, self.flags = int(index), int(log_term), int(flags)

    def __repr__(self):
        return (f"Msg(type={self.type}, frm={self.frm}, term={self.term}, index={self.index}, "
                f"log_term={self.log_term}, flags={self.flags})")


# ---- quorum ----
def majority_vote(member, voted, granted):  # majority.go:178-210
    ids = [s for s in range(16) if member >> s & 1]
    if not ids:
        return VOTE_WON
    yes = sum(1 for s in ids if voted >> s & 1 and granted >> s & 1)
    no = sum(1 for s in ids if voted >> s & 1 and not granted >> s & 1)
    missing = len(ids) - yes - no
    q = len(ids) // 2 + 1
    if yes >= q:
        return VOTE_WON
    if yes + missing >= q:
        return VOTE_PENDING
    return VOTE_LOST


def joint_vote(inc, out, voted, granted):  # joint.go:61-75
    r1, r2 = majority_vote(inc, voted, granted), majority_vote(out, voted, granted)
    if r1 == r2:
        return r1
    if VOTE_LOST in (r1, r2):
        return VOTE_LOST
    return VOTE_PENDING


class _Raft:
    """One Step on a copy of the node."""

    def __init__(self, node, flags, S, election_timeout, out):
        self.n, self.flags, self.S, self.et, self.o = node, flags, S, election_timeout, out
        self.full = (1 << S) - 1
        self.elections = 0
        self.stepdowns = 0

    def none(self, slot):
        return slot >= self.S

    def inc(self):
        return self.full if self.n.inc is None else self.n.inc & self.full

    def out(self):
        return 0 if self.n.out is None else self.n.out & self.full

    def reset(self, term):  # :590-619
        n = self.n
        if n.term != term:
            n.term = term
            n.vote = NONE_SLOT
        n.lead = NONE_SLOT
        self.o["events"] = TEV_RESET  # both elapsed counters, a new randomized timeout
        n.transferee = NONE_SLOT      # abortLeaderTransfer
        n.voted = n.granted = 0       # ResetVotes

    def become_follower(self, term, lead):  # :686-693
        self.reset(term)
        self.n.lead = lead
        self.n.state = ST_FOLLOWER

    def become_candidate(self):  # :695-707
        self.reset(self.n.term + 1)
        self.n.vote = self.n.self_slot
        self.n.state = ST_CANDIDATE

    def become_pre_candidate(self):  # :709-722
        n = self.n
        n.voted = n.granted = 0
        n.lead = NONE_SLOT
        n.state = ST_PRE_CANDIDATE

    def become_leader(self):  # :724-759, the header part
        self.reset(self.n.term)
        self.n.lead = self.n.self_slot
        self.n.state = ST_LEADER
        self.o.update(result=VR_WON, elected=1)

    def poll(self, slot, v):  # :837-845, RecordVote / TallyVotes
        n = self.n
        if not self.none(slot) and not n.voted >> slot & 1:
            n.voted |= 1 << slot
            if v:
                n.granted |= 1 << slot
        return joint_vote(self.inc(), self.out(), n.voted, n.granted)

    def promotable(self):  # :1618-1621
        n = self.n
        if self.none(n.self_slot):
            return False
        tracked = self.full if n.tracked is None else n.tracked
        return bool(tracked >> n.self_slot & 1) and bool((self.inc() | self.out()) >> n.self_slot & 1)

    def hup(self, t):  # :760-781
        n = self.n
        if n.state == ST_LEADER:
            return
        if not self.promotable():
            return
        if n.no_campaign:
            return
        self.elections += 1
        self.campaign(t)

    def campaign(self, t):  # :785-835
        n = self.n
        if t == CAMPAIGN_PRE_ELECTION:
            self.become_pre_candidate()
            result, term = VR_CAMPAIGN_PREVOTE, n.term + 1
        else:
            self.become_candidate()
            result, term = VR_CAMPAIGN_VOTE, n.term
        if self.poll(n.self_slot, True) == VOTE_WON:
            if t == CAMPAIGN_PRE_ELECTION:
                self.campaign(CAMPAIGN_ELECTION)
            else:
                self.become_leader()
            return
        to = (self.inc() | self.out()) & ~(0 if self.none(n.self_slot) else 1 << n.self_slot)
        self.o.update(result=result, resp_term=term, req_log_term=n.last_term(), req_to=to)

    def step(self, m):
        n, o = self.n, self.o
        stepped = False
        if m.type != VMSG_HUP:  # (a local message: term 0)
            if m.term > n.term:
                if m.type in (VMSG_VOTE, VMSG_PREVOTE):
                    force = bool(m.flags & VMF_FORCE)
                    in_lease = (bool(self.flags & VOTE_CHECK_QUORUM) and not self.none(n.lead) and
                                n.elapsed < self.et)
                    if not force and in_lease:
                        o["result"] = VR_IN_LEASE
                        return
                if m.type == VMSG_PREVOTE:
                    pass
                elif m.type == VMSG_PREVOTE_RESP and not m.flags & VMF_REJECT:
                    pass
                else:
                    self.become_follower(m.term, NONE_SLOT)
                    self.stepdowns += 1
                    stepped = True
            elif m.term < n.term:
                if m.type == VMSG_PREVOTE:  # :907-913
                    o.update(result=VR_REJECT, resp_term=n.term)
                else:
                    o["result"] = VR_IGNORED
                return
        o["result"] = VR_STEPPED_DOWN if stepped else VR_IGNORED
        if m.type == VMSG_HUP:
            pre = bool(self.flags & VOTE_PREVOTE)
            self.hup(CAMPAIGN_PRE_ELECTION if pre else CAMPAIGN_ELECTION)
        elif m.type in (VMSG_VOTE, VMSG_PREVOTE):  # :930-978
            can_vote = (n.vote == m.frm or (self.none(n.vote) and self.none(n.lead)) or
                        (m.type == VMSG_PREVOTE and m.term > n.term))
            up_to_date = (m.log_term > n.last_term() or
                          (m.log_term == n.last_term() and m.index >= n.last_index()))
            if can_vote and up_to_date:
                o.update(result=VR_GRANT, resp_term=m.term)
                if m.type == VMSG_VOTE:
                    if not o["events"]:
                        o["events"] = TEV_HEARD  # electionElapsed = 0
                    n.vote = m.frm
            else:
                o.update(result=VR_REJECT, resp_term=n.term)
        elif n.state in (ST_CANDIDATE, ST_PRE_CANDIDATE):  # stepCandidate
            mine = VMSG_PREVOTE_RESP if n.state == ST_PRE_CANDIDATE else VMSG_VOTE_RESP
            if m.type == mine:
                res = self.poll(m.frm, not m.flags & VMF_REJECT)
                if res == VOTE_WON:
                    if n.state == ST_PRE_CANDIDATE:
                        self.campaign(CAMPAIGN_ELECTION)
                    else:
                        self.become_leader()
                elif res == VOTE_LOST:
                    self.become_follower(n.term, NONE_SLOT)
                    self.stepdowns += 1
                    o["result"] = VR_LOST
                else:
                    o["result"] = VR_PENDING
        elif n.state == ST_FOLLOWER:  # stepFollower
            if m.type == VMSG_TIMEOUT_NOW:
                self.hup(CAMPAIGN_TRANSFER)


def bad_msg(node, m, S, cand, have_self):
    if m.type not in range(1, 7):
        return True
    if m.type != VMSG_HUP and (m.frm >= S or m.term == 0):
        return True
    if m.type in (VMSG_VOTE_RESP, VMSG_PREVOTE_RESP, VMSG_HUP, VMSG_TIMEOUT_NOW):
        if not cand or not have_self:
            return True
    if m.type in (VMSG_HUP, VMSG_TIMEOUT_NOW) and node.self_slot >= S:
        return True
    return False


def step(node, m, flags=0, num_slots=16, election_timeout=10, cand=True, have_self=True):
    """raft.Step for one election message.  Returns (node after, out): `out`
    holds result, events, elected and exactly the other output fields the call
    writes for the group; `elections` / `stepdowns` are the statistics'
    shares.  A group nothing changed in comes back as the same object."""
    out = {"result": VR_NONE, "events": 0, "elected": 0}
    if m.type == VMSG_NONE:
        return node, out
    if bad_msg(node, m, num_slots, cand, have_self):
        out["result"] = VR_BAD_MSG
        return node, out
    n = copy.deepcopy(node)
    if not cand:
        n.voted = n.granted = 0
    r = _Raft(n, flags, num_slots, election_timeout, out)
    r.step(m)
    out["elections"], out["stepdowns"] = r.elections, r.stepdowns
    if not cand:
        n.voted, n.granted = node.voted, node.granted
    if n.key() == node.key():
        return node, out
    return n, out


def group_stats(gid, after, out, cand=True):
    """The share of one group with a message in the statistics vector."""
    r = out["result"]
    s = {STAT_GROUPS: 1, STAT_GRANTED: int(r == VR_GRANT), STAT_REJECTED: int(r == VR_REJECT),
         STAT_VOTE_PENDING: int(r == VR_PENDING), STAT_ELECTIONS: out.get("elections", 0),
         STAT_LEADERS: int(r == VR_WON), STAT_STEPDOWNS: out.get("stepdowns", 0),
         STAT_VIOLATIONS: int(r >= VR_REFUSED)}
    h = mix64(((gid * PHI) & M64) ^ VOTE_SALT ^ (r << 56))
    h = mix64(h ^ after.term)
    h = mix64(h ^ (after.state | after.lead << 8 | after.vote << 16 | out["events"] << 24))
    h = mix64(h ^ ((after.voted | after.granted << 16) if cand else 0))
    s[STAT_CHECKSUM] = h
    return s


def group_hashes(gid, result, term, state, lead, vote, events, voted, granted, cand=True):
    """group_stats' STAT_CHECKSUM, vectorised (the state words are the ones after the step)."""
    u64 = lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731
    head = u64(state) | u64(lead) << np.uint64(8) | u64(vote) << np.uint64(16) | \
        u64(events) << np.uint64(24)
    votes = (u64(voted) | u64(granted) << np.uint64(16)) if cand else np.uint64(0)
    return fm.hash_chain(gid, VOTE_SALT, result, (term, head, votes))


def step_batch(nodes, msgs, flags, num_slots, election_timeout=10, cand=True, have_self=True,
               group_offset=0):
    """-> (nodes after, outs, stats dict)"""
    after, outs, stats = [], [], {}
    for g, (n, m) in enumerate(zip(nodes, msgs)):
        n2, o = step(n, m, flags, num_slots, election_timeout, cand, have_self)
        after.append(n2)
        outs.append(o)
        if m.type != VMSG_NONE:
            for k, v in group_stats(group_offset + g, n2, o, cand).items():
                stats[k] = (stats.get(k, 0) + v) & M64
    return after, outs, stats


# ---------------------------------------------------------------------------
# The random generator (shared by tests/test_vote_model.py and
# tests/test_gpu_vote.py).
# ---------------------------------------------------------------------------
def gen_node(rng, R, S, masks="inc", election_timeout=10):
    """masks: "none" (inc_mask NULL: every slot votes), "inc" or "joint"."""
    b = fm.gen_node(rng, R, S)
    full = (1 << S) - 1
    inc = out = None
    if masks != "none":
        inc = int(rng.integers(1, full + 1))
        if rng.random() < 0.1:
            inc = 1 << int(rng.integers(0, S))  # a single voter
    if masks == "joint":
        out = int(rng.integers(0, full + 1)) if rng.random() < 0.7 else 0
    tracked = None
    if masks != "none":
        tracked = ((inc or 0) | (out or 0) | int(rng.integers(0, full + 1))) & full
        if rng.random() < 0.1:
            tracked &= int(rng.integers(0, full + 1))
    u = rng.random()
    voters = [s for s in range(S) if ((full if inc is None else inc) | (out or 0)) >> s & 1]
    if u < 0.8 and voters:
        self_slot = int(rng.choice(voters))
    elif u < 0.93:
        self_slot = int(rng.integers(0, S))
    else:
        self_slot = int(rng.integers(S, 256))
    state = int(rng.choice([ST_FOLLOWER] * 4 + [ST_CANDIDATE] * 3 + [ST_PRE_CANDIDATE] * 2 +
                           [ST_LEADER]))
    voted = granted = 0
    if state in (ST_CANDIDATE, ST_PRE_CANDIDATE):
        voted = int(rng.integers(0, full + 1)) | (1 << self_slot if self_slot < S else 0)
        granted = voted & (int(rng.integers(0, full + 1)) | (1 << self_slot if self_slot < S else 0))
    elif rng.random() < 0.2:  # stale bits the next reset clears
        voted = int(rng.integers(0, full + 1))
        granted = voted & int(rng.integers(0, full + 1))
    return Node(b.ents, voted=voted, granted=granted,
                elapsed=int(rng.integers(0, 2 * election_timeout + 1)), inc=inc, out=out,
                tracked=tracked, self_slot=self_slot, no_campaign=int(rng.random() < 0.1),
                committed=b.committed, term=b.term, state=state, lead=b.lead, vote=b.vote,
                transferee=b.transferee, runs=b.runs)


def gen_msg(rng, node, S):
    u = rng.random()
    if u < 0.08:
        return Msg()
    ty = int(rng.choice([VMSG_VOTE] * 3 + [VMSG_PREVOTE] * 3 + [VMSG_VOTE_RESP] * 3 +
                        [VMSG_PREVOTE_RESP] * 3 + [VMSG_HUP] * 2 + [VMSG_TIMEOUT_NOW]))
    # the same message type as the state expects, more often than chance
    if node.state == ST_CANDIDATE and rng.random() < 0.4:
        ty = VMSG_VOTE_RESP
    if node.state == ST_PRE_CANDIDATE and rng.random() < 0.4:
        ty = VMSG_PREVOTE_RESP
    m = Msg(type=ty, flags=int(rng.integers(0, 4)))
    v = rng.random()
    if v < 0.3 and node.vote < S:
        m.frm = node.vote
    elif v < 0.5 and node.lead < S:
        m.frm = node.lead
    else:
        m.frm = int(rng.integers(0, S))
    w = rng.random()
    m.term = node.term
    if w < 0.45:
        m.term = node.term + int(rng.integers(1, 3))
    elif w < 0.60 and node.term:
        m.term = node.term - int(rng.integers(1, min(node.term, 2) + 1))
    if ty == VMSG_HUP:
        m.term = int(rng.integers(0, 3))  # not read
    # a log one entry better or worse than the node's, in index and in term
    m.index = max(0, node.last_index() + int(rng.integers(-1, 2)))
    m.log_term = max(0, node.last_term() + int(rng.integers(-1, 2)))
    if rng.random() < 0.02:
        m.type = int(rng.integers(7, 256))
    if rng.random() < 0.02:
        m.frm = int(rng.integers(S, 256))
    if rng.random() < 0.02:
        m.term = 0
    return m


# ---------------------------------------------------------------------------
# Nodes and messages as the arrays of the ABI.
# ---------------------------------------------------------------------------
def pack_nodes(nodes, R, S, stride, fill=0):
    a = fm.pack_nodes(nodes, R, stride, fill)
    md = np.uint8 if S <= 8 else np.uint16
    a["voted"] = np.array([n.voted for n in nodes], md)
    a["granted"] = np.array([n.granted for n in nodes], md)
    a["timer"] = np.array([min(n.elapsed, 0xFFFF) | 0x5A5A0000 for n in nodes], np.uint32)
    a["self_slot"] = np.array([n.self_slot for n in nodes], np.uint8)
    a["no_campaign"] = np.array([n.no_campaign for n in nodes], np.uint8)
    for k in ("inc", "out", "tracked"):
        vals = [getattr(n, k) for n in nodes]
        assert all(v is None for v in vals) or not any(v is None for v in vals), k
        a[k] = None if (not vals or vals[0] is None) else np.array(vals, md)
    return a


def pack_msgs(msgs):
    return {
        "type": np.array([m.type for m in msgs], np.uint8),
        "from": np.array([m.frm for m in msgs], np.uint8),
        "term": np.array([m.term for m in msgs], np.uint64),
        "index": np.array([m.index for m in msgs], np.uint64),
        "log_term": np.array([m.log_term for m in msgs], np.uint64),
        "flags": np.array([m.flags for m in msgs], np.uint8),
    }


# ---------------------------------------------------------------------------
# The random run of the differential tests: 8 consecutive calls on one
# evolving state.  tests/test_gpu_vote.py makes every call on the device too;
# tests/test_vote_model.py proves from the model's outcomes that the run meets
# every result code.
# ---------------------------------------------------------------------------
RUN_G = 197        # three full tiles and a ragged one
RUN_GOFF = 1 << 33
# (S, log_runs, masks, flags, the Votes rows present, self_slot present)
RUN_CASES = [(3, 1, "none", 0, True, True), (5, 4, "inc", 1, True, True),
             (9, 16, "joint", 3, True, True), (5, 16, "joint", 2, True, True),
             (9, 4, "inc", 0, True, True),
             (3, 16, "inc", 3, False, True), (9, 1, "none", 1, False, False),
             (5, 4, "inc", 3, True, False)]


def random_run(case, stepper=None, calls=8):
    """-> the set of results seen.  stepper(nodes, msgs) -> (nodes after,
    outs) replaces the model's own step_batch."""
    S, R, masks, flags, cand, have_self = case
    rng = np.random.default_rng(9000 + 101 * S + 7 * R + flags + 2 * cand + have_self)
    nodes = [gen_node(rng, R, S, masks) for _ in range(RUN_G)]
    seen = set()
    for _ in range(calls):
        msgs = [gen_msg(rng, n, S) for n in nodes]
        if stepper:
            nodes, outs = stepper(nodes, msgs)
        else:
            nodes, outs, _ = step_batch(nodes, msgs, flags, S, 10, cand, have_self, RUN_GOFF)
        seen |= {o["result"] for o in outs}
    return seen
