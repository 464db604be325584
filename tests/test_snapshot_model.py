"""tests/snapshot_model.py against the reference's own expectations: the
restore / compaction tables transcribed into tests/golden/snapshot_tables.json,
the seven MsgSnap deliveries of the interaction traces, and the mask rule of
qe_snapshot_step against the Changer-based model over every ConfState of
three slots.  No GPU."""
import copy
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import follower_model as fm
from tests import snapshot_model as sm
from tests.trace_replay import traces

S_FIX = 4  # slot = id - 1 for the fixture's ids 1..4


def tables():
    with open(os.path.join(os.path.dirname(__file__), "golden", "snapshot_tables.json")) as f:
        return json.load(f)


def slots(ids):
    return sm.to_mask(i - 1 for i in ids)


def snap_msg(snap, frm=0, term=0, S=S_FIX):
    return sm.SMsg(sm.SMSG_SNAP, frm, term, snap["index"], snap["term"], slots(snap.get("voters", [])),
                   slots(snap.get("voters_outgoing", [])), slots(snap.get("learners", [])),
                   slots(snap.get("learners_next", [])), int(snap.get("auto_leave", False)),
                   ids=[s + 1 for s in range(S)])


def fresh(node_id, peers, learners, log=(), commit=0, term=0, S=S_FIX):
    """newTestRaft(id, ...) on a storage with those peers: an empty log at
    term 0, a follower."""
    conf = sm.Conf(S, slots(peers), 0, slots(learners),
                   ids=[s + 1 if s + 1 in list(peers) + list(learners) else 0 for s in range(S)])
    node = fm.Node([(0, 0)] + [tuple(e) for e in log], committed=commit, term=term)
    return sm.SNode(node, conf, node_id - 1, 0)


def fixture_cases():
    """(id, SNode before, SMsg) of every message row of the fixture."""
    t, out = tables(), []
    for row in t["restore"]:
        sn = fresh(row["id"], row["peers"], row["learners"])
        out.append((row["name"], sn, snap_msg(row["snapshot"])))
        after, _ = sm.step(sn, snap_msg(row["snapshot"]), S_FIX)
        out.append((row["name"] + ":again", after, snap_msg(row["snapshot"])))
    ig = t["TestRestoreIgnoreSnapshot"]
    sn = fresh(ig["id"], ig["peers"], [], ig["log"], ig["commit"])
    for k, st in enumerate(ig["steps"]):
        m = snap_msg(st["snapshot"])
        out.append((f"TestRestoreIgnoreSnapshot#{k}", sn, m))
        sn, _ = sm.step(sn, m, S_FIX)
    fs = t["TestRestoreFromSnapMsg"]
    out.append(("TestRestoreFromSnapMsg", fresh(fs["id"], fs["peers"], []),
                snap_msg(fs["snapshot"], fs["msg"]["from"] - 1, fs["msg"]["term"])))
    return out


def test_restore_tables():
    for row in tables()["restore"]:
        sn = fresh(row["id"], row["peers"], row["learners"])
        m = snap_msg(row["snapshot"])
        after, out = sm.step(sn, m, S_FIX)
        w = row["want"]
        assert (out["result"] == sm.SR_RESTORED) == w["ok"], row["name"]
        n, c = after.node, after.conf
        assert out["resp_index"] == n.last_index()
        if "last_index" in w:
            assert n.last_index() == w["last_index"], row["name"]
        if "term_at_index" in w:
            assert n.log_term(row["snapshot"]["index"]) == w["term_at_index"], row["name"]
        if "voters" in w:
            assert c.inc == slots(w["voters"]), row["name"]
        if "voter_nodes" in w:  # ProgressTracker.VoterNodes: both halves
            assert c.inc | c.out == slots(w["voter_nodes"]), row["name"]
        if "learners" in w:
            assert c.learner == slots(w["learners"]), row["name"]
        if "is_learner" in w:
            assert c.is_learner == slots(w["is_learner"]), row["name"]
        if "first_index" in w:
            assert (after.first(), after.first_index) == (w["first_index"],) * 2
            assert n.committed == w["committed"] and len(n.ents) - 1 == w["entries"]
        assert after.snap_index == row["snapshot"]["index"]
        # the kernel's rows agree with the Changer's result
        assert not sm.mask_rule(m, S_FIX) and sm.mask_conf(m, S_FIX) == c, row["name"]
        if "again_ok" in w:
            again, out2 = sm.step(after, m, S_FIX)
            assert (out2["result"] == sm.SR_RESTORED) == w["again_ok"]
            assert out2["result"] == sm.SR_STALE and out2["resp_index"] == n.committed
            assert again.node.ents == n.ents and again.conf == c


def test_restore_ignore_snapshot():
    ig = tables()["TestRestoreIgnoreSnapshot"]
    sn = fresh(ig["id"], ig["peers"], [], ig["log"], ig["commit"])
    results = []
    for st in ig["steps"]:
        sn2, out = sm.step(sn, snap_msg(st["snapshot"]), S_FIX)
        assert (out["result"] == sm.SR_RESTORED) == st["want_ok"]
        assert sn2.node.committed == st["want_commit"] == out["resp_index"]
        assert sn2.node.ents == sn.node.ents and sn2.conf == sn.conf
        results.append(out["result"])
        sn = sn2
    assert results == [sm.SR_STALE, sm.SR_FAST_FORWARD]


def test_restore_from_snap_msg():
    fs = tables()["TestRestoreFromSnapMsg"]
    sn = fresh(fs["id"], fs["peers"], [])
    m = snap_msg(fs["snapshot"], fs["msg"]["from"] - 1, fs["msg"]["term"])
    after, out = sm.step(sn, m, S_FIX)
    assert after.node.lead + 1 == fs["want_lead"]
    assert (out["result"], out["events"]) == (sm.SR_RESTORED, fm.TEV_RESET)
    assert (after.node.term, after.node.vote) == (fs["msg"]["term"], fm.NONE_SLOT)


def storage(ents, committed=None, snap_index=0):
    ents = [tuple(e) for e in ents]
    node = fm.Node(ents, committed=ents[-1][0] if committed is None else committed)
    return sm.SNode(node, sm.Conf(3, 1), 0, snap_index)


def test_storage_compact():
    t = tables()["TestStorageCompact"]
    for row in t["rows"]:
        sn = storage(t["ents"])
        after, out = sm.compact(sn, ci=row["i"])
        want = sm.CP_ALREADY if row["werr"] == "ErrCompacted" else sm.CP_COMPACTED
        assert out["result"] == want, row
        assert after.node.ents[0] == (row["windex"], row["wterm"]), row
        assert len(after.node.ents) == row["wlen"], row
        assert after.node.runs[0] == (row["windex"], row["wterm"])
        if want == sm.CP_COMPACTED:
            assert after.first_index == row["i"] + 1


def test_storage_create_snapshot():
    t = tables()["TestStorageCreateSnapshot"]
    for row in t["rows"]:
        after, out = sm.compact(storage(t["ents"]), si=row["i"])
        assert out["result"] == sm.CP_CREATED and row["werr"] is None
        assert (after.snap_index, out["snap_term"]) == (row["windex"], row["wterm"])
        assert after.node.ents == storage(t["ents"]).node.ents  # the log is not touched
        _, again = sm.compact(after, si=row["i"])  # ErrSnapOutOfDate (storage.go:197-199)
        assert again["result"] == sm.CP_SNAP_OUT_OF_DATE


def compaction_cases():
    """(name, storage, [(compact index, entries left or -1)])"""
    out = []
    for k, row in enumerate(tables()["TestCompaction"]["rows"]):
        sn = storage([(i, 0) for i in range(row["last_index"] + 1)])
        out.append((f"TestCompaction#{k}", sn, list(zip(row["compact"], row["wleft"])), row["wallow"]))
    return out


def test_compaction():
    for name, sn, seq, allow in compaction_cases():
        failed = False
        for ci, left in seq:
            after, out = sm.compact(sn, ci=ci, applied=sn.node.committed)
            if out["result"] != sm.CP_COMPACTED:  # a panic or ErrCompacted
                assert left == -1, (name, ci)
                assert out["result"] in (sm.CP_OUT_OF_BOUND, sm.CP_ALREADY)
                assert after is sn
                failed = True
                continue
            assert len(after.node.ents) - 1 == left, (name, ci)
            sn = after
        assert failed == (not allow), name


def test_compaction_side_effects():
    t = tables()["TestCompactionSideEffects"]
    last, off = t["last_index"], t["compact"]
    sn = storage([(0, 0)] + [(i, i) for i in range(1, last + 1)])
    after, out = sm.compact(sn, ci=off, applied=last)
    assert out["result"] == sm.CP_COMPACTED and out["rstar"] == off
    n = after.node
    assert n.last_index() == t["want"]["last_index"] and after.first() == t["want"]["first_index"]
    for j in range(t["want"]["term_of_j_is_j_from"], last + 1):
        assert n.log_term(j) == j and n.match_term(j, j)
    assert n.log_term(off - 1) == 0  # compacted away
    assert (n.committed, sn.node.committed) == (last, last)


# ---------------------------------------------------------------------------
# the interaction traces
# ---------------------------------------------------------------------------
CONF_LINE = re.compile(r"switched to configuration voters=\(([\d ]*)\)(?:&&\(([\d ]*)\))?"
                       r"(?: learners=\(([\d ]*)\))?(?: learners_next=\(([\d ]*)\))?( autoleave)?$")


def trace_cases():
    """The MsgSnap deliveries of tests/golden/interaction_traces.json: (id,
    SNode before, SMsg, the trace's configuration line, the index of the
    MsgAppResp the receiver's next Ready carries).  The message's ConfState is
    the one its "switched to configuration" line prints: the reference asserts
    the two equivalent (raft.go:1606), so the line determines it.  The
    receiver's log before is the one its "starts to restore" line prints."""
    S, out = 7, []
    for name, tr in traces().items():
        owed = {}  # node -> the MsgApp / MsgSnap it received since its last Ready
        for c in tr["commands"]:
            for b in c["blocks"]:
                n = b["node"]
                if b["kind"] == "status":
                    continue
                if b["kind"] != "recv":
                    resps = [m for m in b["msgs"] if m["type"] == "MsgAppResp"]
                    for pos, case in owed.pop(n, []):
                        if case is not None:
                            case.append(resps[pos]["index"])
                    continue
                for m in b["msgs"]:
                    if m["type"] == "MsgApp":
                        owed.setdefault(n, []).append((len(owed.get(n, [])), None))
                    if m["type"] != "MsgSnap":
                        continue
                    dbg = b["debug"]
                    log = [re.search(r"log \[committed=(\d+), applied=\d+, unstable.offset=(\d+), "
                                     r"len\(unstable.Entries\)=(\d+)\] starts to restore snapshot "
                                     r"\[index: (\d+), term: (\d+)\]", d) for d in dbg]
                    com, offset, ln, idx, term = map(int, [x for x in log if x][0].groups())
                    assert idx == m["snap_index"] and ln == 0 and offset == 1
                    line = [d for d in dbg if "switched to configuration" in d][0]
                    v, o, l, ln_, auto = CONF_LINE.search(line).groups()
                    ids = lambda s: [int(x) for x in (s or "").split()]  # noqa: E731
                    down = any(f"became follower at term {m['term']}" in d for d in dbg)
                    node = fm.Node([(0, 0)], committed=com, term=m["term"] - 1 if down else m["term"])
                    sn = sm.SNode(node, sm.Conf(S), n - 1, 0)
                    msg = sm.SMsg(sm.SMSG_SNAP, m["from"] - 1, m["term"], idx, term, slots(ids(v)),
                                  slots(ids(o)), slots(ids(l)), slots(ids(ln_)), int(bool(auto)),
                                  ids=[s + 1 for s in range(S)])
                    case = [f"{name}:{c['line']}:n{n}", sn, msg,
                            line[line.index("voters="):]]
                    owed.setdefault(n, []).append((len(owed.get(n, [])), case))
                    out.append(case)
    return [tuple(c) for c in out]


def test_trace_deliveries():
    cases = trace_cases()
    assert len(cases) == 7  # none skipped
    lines = set()
    for cid, sn, m, line, resp in cases:
        after, out = sm.step(sn, m, 7)
        assert out["result"] == sm.SR_RESTORED, cid
        assert after.conf.string() == line, cid
        assert out["resp_index"] == resp == m.sindex, cid
        assert (after.node.committed, after.node.last_index()) == (m.sindex, m.sindex)
        assert not sm.mask_rule(m, 7) and sm.mask_conf(m, 7) == after.conf
        lines.add(line)
    assert {"voters=(1 2)&&(1) autoleave", "voters=(1 2 3)&&(1) autoleave"} <= lines


# ---------------------------------------------------------------------------
# the mask rule against the Changer, exhaustively for three slots
# ---------------------------------------------------------------------------
def test_mask_rule_exhaustive_three_slots():
    S, n_bad = 3, 0
    for inc, out, lrn, lnx, auto in itertools.product(range(8), range(8), range(8), range(8),
                                                      (0, 1)):
        m = sm.SMsg(sm.SMSG_SNAP, 0, 1, 5, 5, inc, out, lrn, lnx, auto, ids=[11, 12, 13])
        try:
            want = sm.restore_config(m, S)
        except sm.Refused as e:
            assert e.code == sm.SR_BAD_CONF
            want = None
        assert sm.mask_rule(m, S) == (want is None), (inc, out, lrn, lnx, auto)
        if want is None:
            n_bad += 1
        else:
            assert sm.mask_conf(m, S) == want, (inc, out, lrn, lnx, auto)
    assert 0 < n_bad < 8192


def test_preamble_lower_term_is_always_ignored():
    """The one difference from qe_follower_step: :884 lists MsgApp and
    MsgHeartbeat only, so a lower-term MsgSnap gets no response."""
    node = fm.Node([(0, 0)], term=5, lead=1)
    sn = sm.SNode(node, sm.Conf(3, 7), 0, 0)
    m = sm.SMsg(sm.SMSG_SNAP, 1, 4, 9, 4, 7)
    after, out = sm.step(sn, m, 3)
    assert after is sn and out == {"result": sm.SR_IGNORED, "events": 0}


def test_random_model_walk():
    """The generators reach every result, and the model's own invariants
    (the expanded run table equals the entries) hold across compact ->
    restore -> compact."""
    rng = np.random.default_rng(3)
    seen_s, seen_c = set(), set()
    for S, R in ((3, 4), (9, 5), (16, 16)):
        nodes = [sm.gen_snode(rng, R, S) for _ in range(400)]
        for _ in range(2):
            nodes, outs, _ = sm.compact_batch(nodes, [sm.gen_compaction(rng, n) for n in nodes])
            seen_c |= {o["result"] for o in outs}
            nodes, outs, _ = sm.step_batch(nodes, [sm.gen_smsg(rng, n, S) for n in nodes], S, R)
            seen_s |= {o["result"] for o in outs}
            for n in nodes:
                n.node.check()
                assert n.node.ents[0][0] <= n.node.committed <= n.node.last_index()
    assert seen_s == set(sm.SR_NAMES), sorted(set(sm.SR_NAMES) - seen_s)
    assert {sm.CP_NONE, sm.CP_CREATED, sm.CP_COMPACTED, sm.CP_CREATED | sm.CP_COMPACTED,
            sm.CP_ALREADY, sm.CP_SNAP_OUT_OF_DATE, sm.CP_OUT_OF_BOUND,
            sm.CP_PAST_APPLIED} <= seen_c


# ---------------------------------------------------------------------------
# negative controls: each must fail
# ---------------------------------------------------------------------------
def test_negative_control_changed_snapshot_term():
    row = tables()["restore"][0]
    snap = dict(row["snapshot"], term=row["snapshot"]["term"] + 1)
    after, _ = sm.step(fresh(row["id"], row["peers"], row["learners"]), snap_msg(snap), S_FIX)
    with pytest.raises(AssertionError):
        assert after.node.log_term(snap["index"]) == row["want"]["term_at_index"]


def test_negative_control_dropped_learner_bit():
    row = [r for r in tables()["restore"] if r["name"] == "TestRestoreWithLearner"][0]
    m = snap_msg(row["snapshot"])
    want = sm.restore_config(m, S_FIX)
    broken = copy.copy(m)
    broken.learner = 0  # the kernel's rows with the bit lost
    with pytest.raises(AssertionError):
        assert sm.mask_conf(broken, S_FIX) == want


def test_negative_control_compaction_index_off_by_one():
    t = tables()["TestStorageCompact"]
    row = t["rows"][2]
    after, _ = sm.compact(storage(t["ents"]), ci=row["i"] + 1)
    with pytest.raises(AssertionError):
        assert after.node.ents[0] == (row["windex"], row["wterm"])
