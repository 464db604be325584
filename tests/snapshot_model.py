"""CPU model of qe_snapshot_step and qe_compact: the reference restated
sequentially on tests/follower_model.Node (an explicit list of (index, term)
entries) plus the group's configuration.

  step()     raft.Step's term preamble for a MsgSnap (raft/raft.go:849-920),
             the MsgSnap arms of stepFollower / stepCandidate (:1396-1398,
             :1441-1444), handleSnapshot / restore (:1518-1614) and
             raftLog.restore (raft/log.go:333-337).  The restored configuration
             goes through oracle/confchange_ref.Changer exactly as
             confchange.Restore chains it (raft/confchange/restore.go:21-155:
             one Simple per change, or the outgoing voters one by one followed
             by EnterJoint), then the ConfState equivalence check of
             assertConfStatesEquivalent.  Nothing here uses the mask rule the
             kernel implements; mask_rule() / mask_conf() restate that rule for
             the exhaustive comparison only.
  compact()  MemoryStorage.CreateSnapshot / Compact (raft/storage.go:194-236)
             on the entry list; the run table is bookkeeping next to it, moved
             by the rule include/etcd_quorum.h states, and after every step the
             expanded table must equal the entry list.

Also here: the random generators the CPU and the GPU tests share and the
packing of nodes and messages into the arrays of the ABI.
"""
import copy

import numpy as np

from oracle import confchange_ref as cc
from tests import follower_model as fm
from tests.follower_model import M64, NONE_SLOT, PHI, mix64

SMSG_NONE, SMSG_SNAP = 0, 1
SR_NONE, SR_IGNORED, SR_STALE, SR_NOT_MEMBER, SR_FAST_FORWARD, SR_RESTORED = 0, 1, 2, 3, 4, 5
SR_REFUSED = 16
SR_BAD_MSG, SR_COMMIT_PAST_LOG, SR_BAD_CONF = 16, 17, 18
SR_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("SR_") and k != "SR_REFUSED"}

CP_NONE, CP_CREATED, CP_COMPACTED, CP_SNAP_OUT_OF_DATE, CP_ALREADY = 0, 1, 2, 4, 8
CP_REFUSED = 16
CP_OUT_OF_BOUND, CP_PAST_APPLIED = 16, 17

STAT_GROUPS, STAT_COMPACTED, STAT_GRANTED, STAT_REJECTED = 0, 2, 7, 8
STAT_COMMIT_ADVANCED, STAT_VIOLATIONS, STAT_CHECKSUM = 9, 14, 15
SNAP_SALT, COMPACT_SALT = 0x8CB92BA72F3D8DD7, 0xD1B54A32D192ED03

CONF_MASKS = ("inc", "out", "learner", "learners_next", "is_learner", "tracked")


class Refused(Exception):
    """A panic of the reference (or input the ABI refuses): the step is undone."""

    def __init__(self, code):
        super().__init__(str(code))
        self.code = code


def bits(mask):
    return [s for s in range(32) if (mask >> s) & 1]


def to_mask(slots):
    m = 0
    for s in slots:
        m |= 1 << s
    return m


class Conf:
    """tracker.Config + the ProgressMap's keys and IsLearner in slot form (the
    rows of qe_conf); ids[s] is the peer id of slot s (0 = none)."""

    def __init__(self, S, inc=0, out=0, learner=0, learners_next=0, is_learner=None, tracked=None,
                 auto_leave=0, ids=None):
        self.S = S
        self.inc, self.out, self.learner, self.learners_next = inc, out, learner, learners_next
        self.is_learner = learner if is_learner is None else is_learner
        self.tracked = (inc | out | learner) if tracked is None else tracked
        self.auto_leave = int(auto_leave)
        self.ids = list(ids) if ids is not None else [0] * S

    def key(self):
        return tuple(getattr(self, k) for k in CONF_MASKS) + (self.auto_leave, tuple(self.ids))

    def __eq__(self, other):
        return self.key() == other.key()

    def string(self, ids=None):
        """tracker.Config.String through confchange_ref, ids[s] naming slot s."""
        ids = ids or [s + 1 for s in range(self.S)]
        c = cc.Config()
        c.inc = {ids[s] for s in bits(self.inc)}
        c.out = {ids[s] for s in bits(self.out)}
        c.learners = {ids[s] for s in bits(self.learner)}
        c.lnext = {ids[s] for s in bits(self.learners_next)}
        c.auto_leave = bool(self.auto_leave)
        return c.string()


class SNode:
    """A raft group as the receiver of a MsgSnap and as the owner of its
    storage: the log (follower_model.Node), the configuration, the node's own
    slot, and the index of the snapshot MemoryStorage holds."""

    def __init__(self, node, conf, self_slot=0, snap_index=0):
        self.node, self.conf = node, conf
        self.self_slot, self.snap_index = int(self_slot), int(snap_index)
        self.first_index = node.ents[0][0] + 1

    def first(self):  # raftLog.firstIndex()
        return self.node.ents[0][0] + 1


class SMsg:
    """One MsgSnap: the ConfState as slot masks in the receiver's numbering."""

    def __init__(self, type=SMSG_NONE, frm=0, term=0, sindex=0, sterm=0, inc=0, out=0, learner=0,
                 learners_next=0, auto_leave=0, ids=None):
        self.type, self.frm, self.term = int(type), int(frm), int(term)
        self.sindex, self.sterm = int(sindex), int(sterm)
        self.inc, self.out, self.learner = int(inc), int(out), int(learner)
        self.learners_next, self.auto_leave = int(learners_next), int(auto_leave)
        self.ids = ids


# ---------------------------------------------------------------------------
# confchange.Restore through the Changer
# ---------------------------------------------------------------------------
def restore_config(m, S, last_index=0):
    """raft/confchange/restore.go:21-155 then assertConfStatesEquivalent
    (raft/raft.go:1606) -> Conf; Refused(SR_BAD_CONF) where the reference
    panics.  A bit at or past S names no peer: the ABI refuses it."""
    if (m.inc | m.out | m.learner | m.learners_next) >> S:
        raise Refused(SR_BAD_CONF)
    ids = list(m.ids) if m.ids is not None else [s + 1 for s in range(S)]
    voters = [ids[s] for s in bits(m.inc)]
    learners = [ids[s] for s in bits(m.learner)]
    outgoing_v = [ids[s] for s in bits(m.out)]
    lnext = [ids[s] for s in bits(m.learners_next)]
    # toConfChangeSingle (:25-89)
    outgoing = [(cc.ADD_NODE, i) for i in outgoing_v]
    incoming = ([(cc.REMOVE_NODE, i) for i in outgoing_v] + [(cc.ADD_NODE, i) for i in voters] +
                [(cc.ADD_LEARNER_NODE, i) for i in learners] +
                [(cc.ADD_LEARNER_NODE, i) for i in lnext])
    chg = cc.Changer(last_index=last_index)
    try:
        if not outgoing:  # :120-127
            for c in incoming:
                chg.cfg, chg.prs = chg.simple([c])
        else:  # :128-151
            for c in outgoing:
                chg.cfg, chg.prs = chg.simple([c])
            chg.cfg, chg.prs = chg.enter_joint(bool(m.auto_leave), incoming)
    except cc.ChangeError:
        raise Refused(SR_BAD_CONF) from None
    cfg, prs = chg.cfg, chg.prs
    # ProgressTracker.ConfState() against the message's (sorted, as the check does)
    same = (sorted(cfg.inc) == sorted(voters) and sorted(cfg.out) == sorted(outgoing_v) and
            sorted(cfg.learners) == sorted(learners) and sorted(cfg.lnext) == sorted(lnext) and
            bool(cfg.auto_leave) == bool(m.auto_leave))
    if not same:
        raise Refused(SR_BAD_CONF)
    slot = {i: s for s, i in enumerate(ids) if (m.inc | m.out | m.learner | m.learners_next) >> s & 1}
    mk = lambda idset: to_mask(slot[i] for i in idset)  # noqa: E731
    tracked = mk(prs.keys())
    return Conf(S, mk(cfg.inc), mk(cfg.out), mk(cfg.learners), mk(cfg.lnext),
                is_learner=mk(i for i, p in prs.items() if p.is_learner), tracked=tracked,
                auto_leave=int(cfg.auto_leave),
                ids=[ids[s] if tracked >> s & 1 else 0 for s in range(S)])


def mask_rule(m, S):
    """The kernel's rule of step 7 (include/etcd_quorum.h): True = QE_SR_BAD_CONF."""
    full = (1 << S) - 1
    return bool((m.inc == 0 and (m.out | m.learner)) or (m.inc | m.out) & m.learner or m.learners_next & ~(m.out & ~m.inc)
                or (m.out == 0 and (m.learners_next or m.auto_leave))
                or (m.inc | m.out | m.learner | m.learners_next) & ~full)


def mask_conf(m, S):
    """The rows step 8 writes, in mask form."""
    ids = list(m.ids) if m.ids is not None else [s + 1 for s in range(S)]
    trk = m.inc | m.out | m.learner
    return Conf(S, m.inc, m.out, m.learner, m.learners_next, is_learner=m.learner, tracked=trk,
                auto_leave=int(bool(m.auto_leave)),
                ids=[ids[s] if trk >> s & 1 else 0 for s in range(S)])


# ---------------------------------------------------------------------------
# raft.Step for one MsgSnap
# ---------------------------------------------------------------------------
def step(sn, m, num_slots=16, log_runs=16):
    """-> (SNode after, out): `out` holds `result`, `events` and exactly the
    output fields the call writes for the group."""
    out = {"result": SR_NONE, "events": 0}
    if m.type == SMSG_NONE:
        return sn, out
    if m.type != SMSG_SNAP or m.frm >= num_slots or m.sindex >= M64:  # 2^64 - 1: no log index
        out["result"] = SR_BAD_MSG
        return sn, out
    node = sn.node
    if m.term < node.term:  # :883-919: only MsgApp / MsgHeartbeat are answered
        out["result"] = SR_IGNORED
        return sn, out
    n = copy.deepcopy(node)
    if m.term > n.term:  # :876-877
        n.become_follower(m.term, m.frm)
        out["events"] = fm.TEV_RESET
    elif n.state == fm.ST_LEADER:  # stepLeader has no MsgSnap arm
        out["result"] = SR_IGNORED
        return sn, out
    elif n.state in (fm.ST_CANDIDATE, fm.ST_PRE_CANDIDATE):  # :1396-1398
        n.become_follower(m.term, m.frm)
        out["events"] = fm.TEV_RESET
    else:  # :1441-1444
        n.lead = m.frm
        out["events"] = fm.TEV_HEARD
    new = SNode(n, sn.conf, sn.self_slot, sn.snap_index)
    new.first_index = sn.first_index
    try:
        # handleSnapshot (:1518-1529) / restore (:1534-1614)
        if m.sindex <= n.committed:
            out.update(result=SR_STALE, resp_index=n.committed)
            return new, out
        assert n.state == fm.ST_FOLLOWER
        selfb = 1 << sn.self_slot if sn.self_slot < num_slots else 0
        if not selfb & (m.inc | m.learner | m.out):
            out.update(result=SR_NOT_MEMBER, resp_index=n.committed)
            return new, out
        if n.match_term(m.sindex, m.sterm):
            if n.last_index() < m.sindex:  # commitTo's panic (log.go:236-238)
                raise Refused(SR_COMMIT_PAST_LOG)
            n.commit_to(m.sindex)
            out.update(result=SR_FAST_FORWARD, resp_index=n.committed)
            return new, out
        # raftLog.restore: committed = index, the log is the snapshot alone
        n.ents = [(m.sindex, m.sterm)]
        n.runs = [(m.sindex, m.sterm)]
        n.committed = m.sindex
        new.conf = restore_config(m, num_slots, n.last_index())
        new.first_index = m.sindex + 1
        new.snap_index = m.sindex
        n.check()
        out.update(result=SR_RESTORED, resp_index=n.last_index())
        return new, out
    except Refused as e:
        return sn, {"result": e.code, "events": 0}


def step_stats(gid, before, after, out):
    r = out["result"]
    s = {STAT_GROUPS: 1, STAT_GRANTED: int(r == SR_RESTORED),
         STAT_REJECTED: int(r in (SR_STALE, SR_NOT_MEMBER)),
         STAT_COMMIT_ADVANCED: int(after.node.committed > before.node.committed),
         STAT_VIOLATIONS: int(r >= SR_REFUSED)}
    h = mix64(((gid * PHI) & M64) ^ SNAP_SALT ^ (r << 56))
    h = mix64(h ^ after.node.term)
    h = mix64(h ^ after.node.committed)
    h = mix64(h ^ after.node.last_index())
    s[STAT_CHECKSUM] = h
    return s


def step_hashes(gid, result, term, committed, last_index):
    """step_stats' STAT_CHECKSUM, vectorised (the state words are the ones after the step)."""
    return fm.hash_chain(gid, SNAP_SALT, result, (term, committed, last_index))


def step_batch(nodes, msgs, num_slots, log_runs, group_offset=0):
    after, outs, stats = [], [], {}
    for g, (sn, m) in enumerate(zip(nodes, msgs)):
        n2, o = step(sn, m, num_slots, log_runs)
        after.append(n2)
        outs.append(o)
        if m.type != SMSG_NONE:
            for k, v in step_stats(group_offset + g, sn, n2, o).items():
                stats[k] = (stats.get(k, 0) + v) & M64
    return after, outs, stats


# ---------------------------------------------------------------------------
# MemoryStorage.CreateSnapshot / Compact
# ---------------------------------------------------------------------------
def compact(sn, ci=0, si=0, applied=None):
    """-> (SNode after, out): create then compact; `out` holds `result`,
    `snap_term` where a snapshot was created and `compacted` (entries)."""
    out = {"result": CP_NONE}
    if ci == 0 and si == 0:
        return sn, out
    node = sn.node
    new = SNode(copy.deepcopy(node), sn.conf, sn.self_slot, sn.snap_index)
    new.first_index = sn.first_index
    n = new.node
    offset, last = n.ents[0][0], n.last_index()
    bound = n.committed if applied is None else min(applied, n.committed)
    res = 0
    try:
        if si:  # storage.go:194-213
            if si <= sn.snap_index:
                res |= CP_SNAP_OUT_OF_DATE
            elif si > last or si < offset:
                raise Refused(CP_OUT_OF_BOUND)
            elif si > bound:
                raise Refused(CP_PAST_APPLIED)
            else:
                new.snap_index = si
                out["snap_term"] = n.ents[si - offset][1]
                res |= CP_CREATED
        if ci:  # storage.go:218-236
            if ci <= offset:
                res |= CP_ALREADY
            elif ci > last:
                raise Refused(CP_OUT_OF_BOUND)
            elif ci > bound:
                raise Refused(CP_PAST_APPLIED)
            else:
                i = ci - offset
                n.ents = [n.ents[i]] + n.ents[i + 1:]
                # the run table, by the ABI's rule
                rstar = max(r for r, (f, _) in enumerate(n.runs) if f <= ci)
                n.runs = [(ci, n.runs[rstar][1])] + n.runs[rstar + 1:]
                new.first_index = ci + 1
                out["compacted"] = ci - offset
                out["rstar"] = rstar
                res |= CP_COMPACTED
    except Refused as e:
        return sn, {"result": e.code}
    n.check()
    out["result"] = res
    if not res & (CP_CREATED | CP_COMPACTED):
        return sn, out
    return new, out


def compact_stats(gid, after, out, have_snap=True):
    r = out["result"]
    s = {STAT_GROUPS: 1, STAT_COMPACTED: out.get("compacted", 0),
         STAT_VIOLATIONS: int(r >= CP_REFUSED)}
    h = mix64(((gid * PHI) & M64) ^ COMPACT_SALT ^ (r << 56))
    h = mix64(h ^ after.node.ents[0][0])
    h = mix64(h ^ len(after.node.runs))
    h = mix64(h ^ (after.snap_index if have_snap else 0))
    s[STAT_CHECKSUM] = h
    return s


def compact_hashes(gid, result, dummy_index, run_count, snap_index):
    """compact_stats' STAT_CHECKSUM, vectorised: the dummy entry's index, the
    run count and the snapshot index (0 without the row) after the call."""
    return fm.hash_chain(gid, COMPACT_SALT, result, (dummy_index, run_count, snap_index))


def compact_batch(nodes, reqs, group_offset=0, have_snap=True):
    """reqs: (ci, si, applied) per group."""
    after, outs, stats = [], [], {}
    for g, (sn, (ci, si, ap)) in enumerate(zip(nodes, reqs)):
        n2, o = compact(sn, ci, si, ap)
        after.append(n2)
        outs.append(o)
        if ci or si:
            for k, v in compact_stats(group_offset + g, n2, o, have_snap).items():
                stats[k] = (stats.get(k, 0) + v) & M64
    return after, outs, stats


# ---------------------------------------------------------------------------
# The random generators (shared by the CPU and the GPU tests).
# ---------------------------------------------------------------------------
def gen_valid_cs(rng, S, must=None):
    """A ConfState confchange.Restore accepts, as masks."""
    full = (1 << S) - 1
    inc = int(rng.integers(1, full + 1))
    out = lnx = auto = 0
    if rng.random() < 0.4:
        out = int(rng.integers(1, full + 1))
        lnx = int(rng.integers(0, full + 1)) & out & ~inc
        auto = int(rng.random() < 0.5)
    learner = int(rng.integers(0, full + 1)) & ~(inc | out) if rng.random() < 0.5 else 0
    if must is not None and must < S and not (inc | out | learner) >> must & 1:
        inc |= 1 << must
        lnx &= ~inc
    return inc, out, learner, lnx, auto


def gen_snode(rng, R, S):
    node = fm.gen_node(rng, R, S)
    inc, out, learner, lnx, auto = gen_valid_cs(rng, S)
    trk = inc | out | learner
    conf = Conf(S, inc, out, learner, lnx, auto_leave=auto,
                ids=[100 + s if trk >> s & 1 else 0 for s in range(S)])
    self_slot = int(rng.integers(0, S)) if rng.random() < 0.95 else NONE_SLOT
    return SNode(node, conf, self_slot, int(rng.integers(0, node.ents[0][0] + 1)))


def gen_smsg(rng, sn, S, p_none=0.25):
    node = sn.node
    if rng.random() < p_none:
        return SMsg()
    m = SMsg(SMSG_SNAP, frm=int(rng.integers(0, S)))
    if rng.random() < 0.03:
        m.type = int(rng.integers(2, 256))
    if rng.random() < 0.03:
        m.frm = int(rng.integers(S, 256))
    v = rng.random()
    m.term = node.term
    if v < 0.15:
        m.term = node.term + int(rng.integers(1, 4))
    elif v < 0.25 and node.term:
        m.term = node.term - int(rng.integers(1, node.term + 1))
    last, dummy = node.last_index(), node.ents[0][0]
    k = rng.random()
    if k < 0.45:  # the usual one: far past the log
        m.sindex, m.sterm = last + int(rng.integers(1, 50)), node.ents[-1][1] + int(rng.integers(0, 3))
        m.sterm = max(m.sterm, 1)
    elif k < 0.57:  # stale
        m.sindex, m.sterm = int(rng.integers(0, node.committed + 1)), int(rng.integers(0, 4))
    elif k < 0.75 and node.committed < last:  # inside the log, the log's term: fast-forward
        m.sindex = int(rng.integers(node.committed + 1, last + 1))
        m.sterm = node.log_term(m.sindex)
    elif k < 0.88 and node.committed < last:  # inside the log, another term
        m.sindex = int(rng.integers(node.committed + 1, last + 1))
        m.sterm = node.log_term(m.sindex) + int(rng.integers(1, 3))
    elif k < 0.94:  # past the log with term 0, which term() "matches"
        m.sindex, m.sterm = last + int(rng.integers(1, 4)), 0
    else:
        m.sindex, m.sterm = last + 1, node.ents[-1][1] + 1
    if rng.random() < 0.88:
        must = sn.self_slot if rng.random() < 0.92 else None
        m.inc, m.out, m.learner, m.learners_next, m.auto_leave = gen_valid_cs(rng, S, must)
    else:  # anything, bits past S included
        top = 1 << (8 if S <= 8 else 16)
        r = lambda: int(rng.integers(0, top)) & (int(rng.integers(0, top)) | (1 << S) - 1)  # noqa: E731
        m.inc, m.out, m.learner, m.learners_next = r(), r() * int(rng.random() < 0.6), r(), r()
        m.learner &= int(rng.integers(0, top))
        m.learners_next &= m.out if rng.random() < 0.5 else top - 1
        m.auto_leave = int(rng.integers(0, 3))
        if rng.random() < 0.5 and sn.self_slot < S:
            m.inc |= 1 << sn.self_slot
    m.ids = [1000 + 7 * s + int(rng.integers(0, 5)) for s in range(S)]
    return m


def gen_compaction(rng, sn, p_none=0.25):
    """-> (ci, si, applied)"""
    n = sn.node
    dummy, last, com = n.ents[0][0], n.last_index(), n.committed
    applied = int(rng.integers(dummy, last + 1)) if rng.random() < 0.5 else com
    bound = min(applied, com)

    def pick(floor):
        k = rng.random()
        if k < 0.15:
            return int(rng.integers(0, floor + 1)) or floor  # at or below the floor
        if k < 0.75 and bound > floor:
            return int(rng.integers(floor + 1, bound + 1))
        if k < 0.85 and last > bound:
            return int(rng.integers(bound + 1, last + 1))  # past applied
        if k < 0.93:
            return last + int(rng.integers(1, 4))  # out of bound
        return int(rng.integers(max(dummy, 1), max(last, dummy, 1) + 1))
    ci = 0 if rng.random() < p_none else pick(dummy)
    si = 0 if rng.random() < 0.5 else pick(sn.snap_index)
    if rng.random() < 0.03 and dummy > 1:
        si = int(rng.integers(1, dummy))  # below the dummy entry
    return ci, si, applied


# ---------------------------------------------------------------------------
# Nodes and messages as the arrays of the ABI.
# ---------------------------------------------------------------------------
def mask_dtype(S):
    return np.uint8 if S <= 8 else np.uint16


def pack_snodes(nodes, R, S, stride, fill=0):
    a = fm.pack_nodes([sn.node for sn in nodes], R, stride, fill)
    md, G = mask_dtype(S), len(nodes)
    a["self_slot"] = np.array([sn.self_slot for sn in nodes], np.uint8)
    a["first_index"] = np.array([sn.first_index for sn in nodes], np.uint64)
    a["snap_index"] = np.array([sn.snap_index for sn in nodes], np.uint64)
    for k in CONF_MASKS:
        a["c_" + k] = np.array([getattr(sn.conf, k) for sn in nodes], md)
    a["c_auto_leave"] = np.array([sn.conf.auto_leave for sn in nodes], np.uint8)
    a["c_slot_ids"] = np.array([[sn.conf.ids[s] for sn in nodes] for s in range(S)],
                               np.uint64).reshape(S * G)
    return a


def pack_smsgs(msgs, S, stride):
    md = mask_dtype(S)
    full = (1 << (8 * np.dtype(md).itemsize)) - 1
    a = {
        "type": np.array([m.type for m in msgs], np.uint8),
        "from": np.array([m.frm for m in msgs], np.uint8),
        "term": np.array([m.term for m in msgs], np.uint64),
        "snap_index": np.array([m.sindex for m in msgs], np.uint64),
        "snap_term": np.array([m.sterm for m in msgs], np.uint64),
        "cs_inc": np.array([m.inc & full for m in msgs], md),
        "cs_out": np.array([m.out & full for m in msgs], md),
        "cs_learner": np.array([m.learner & full for m in msgs], md),
        "cs_learners_next": np.array([m.learners_next & full for m in msgs], md),
        "cs_auto_leave": np.array([m.auto_leave for m in msgs], np.uint8),
        "cs_ids": np.zeros(S * stride, np.uint64),
    }
    for g, m in enumerate(msgs):
        ids = m.ids if m.ids is not None else [s + 1 for s in range(S)]
        for s in range(S):
            a["cs_ids"][s * stride + g] = ids[s]
    return a
