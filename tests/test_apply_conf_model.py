"""tests/apply_conf_model.py (the sequential model of qe_apply_conf) pinned to
the reference's interaction traces (tests/golden/interaction_traces.json).

The fixture holds 28 "switched to configuration" lines.  7 sit in a `recv`
block that delivers a MsgSnap: those are raft.restore, not an applied change;
the node's configuration is set from the printed text.  21 sit in `ready`
blocks: applied conf changes.  For each of them the model applies the
ConfChangeV2 the trace proposed (decode, Changer) to the node's configuration
and must print the line's text; its role outcome must be LEADER exactly where
the node leads.
"""
import json
import os
import re

import pytest

from tests import apply_conf_model as acm
from oracle import confchange_ref as cc

HERE = os.path.dirname(os.path.abspath(__file__))
S = 8

# The set-up of each trace that applies a conf change, restated: the
# configuration its add-nodes command starts every node with, and the leader
# of a trace whose election runs under `log-level none` (so that no
# lead_state line of the fixture shows it).
START = {
    "campaign_learner_must_vote.txt": dict(voters=(1, 2), learners=(3,), nodes=3, leader=1),
    "confchange_v1_add_single.txt": dict(voters=(1,), learners=(), nodes=1, leader=None),
    "confchange_v2_add_single_auto.txt": dict(voters=(1,), learners=(), nodes=1, leader=None),
    "confchange_v2_add_double_implicit.txt": dict(voters=(1,), learners=(), nodes=1, leader=None),
    "confchange_v1_remove_leader.txt": dict(voters=(1, 2, 3), learners=(), nodes=3, leader=1),
    "confchange_v2_add_single_explicit.txt": dict(voters=(1,), learners=(), nodes=1, leader=None),
    "confchange_v2_add_double_auto.txt": dict(voters=(1,), learners=(), nodes=1, leader=None),
}
EXPECT = {"campaign_learner_must_vote.txt": 1, "confchange_v1_add_single.txt": 1,
          "confchange_v2_add_single_auto.txt": 1, "confchange_v2_add_double_implicit.txt": 3,
          "confchange_v1_remove_leader.txt": 3, "confchange_v2_add_single_explicit.txt": 3,
          "confchange_v2_add_double_auto.txt": 9}
SWITCHED = re.compile(r"INFO (\d+) switched to configuration (.*)$")
TRANSITION = {"auto": acm.AUTO, "implicit": acm.JOINT_IMPLICIT, "explicit": acm.JOINT_EXPLICIT}


def traces():
    return json.load(open(os.path.join(HERE, "golden", "interaction_traces.json")))


def changer_from(voters, learners, S=S):
    """A node's start: the ids in ascending slots, voters first."""
    ch = acm.SlotChanger(S)
    for s, i in enumerate(list(voters) + list(learners)):
        ch.slots[i] = s
        ch.prs[i] = cc.Progress(1, i in learners)
    ch.cfg.inc, ch.cfg.learners = set(voters), set(learners)
    return ch


def changer_from_text(text, S=S):
    """A node's configuration after a restore, from Config.String."""
    m = re.match(r"voters=\(([\d ]*)\)(?:&&\(([\d ]*)\))?(?: learners=\(([\d ]*)\))?"
                 r"(?: learners_next=\(([\d ]*)\))?( autoleave)?$", text)
    assert m, text
    inc, out, lrn, lnx = ({int(x) for x in (m.group(k) or "").split()} for k in (1, 2, 3, 4))
    ch = acm.SlotChanger(S)
    for s, i in enumerate(sorted(inc | out | lrn | lnx)):
        ch.slots[i] = s
        ch.prs[i] = cc.Progress(1, i in lrn)
    ch.cfg.inc, ch.cfg.out, ch.cfg.learners, ch.cfg.lnext = inc, out, lrn, lnx
    ch.cfg.auto_leave = bool(m.group(5))
    return ch


def proposal(cmd):
    """An accepted propose-conf-change command -> (transition, changes)."""
    args = cmd["cmd"].split()[2:]
    tr = acm.AUTO
    for a in args:
        if a.startswith("transition="):
            tr = TRANSITION[a.split("=")[1]]
    ccs = [(t, n, acm.ANY_SLOT) for line in cmd["input"] for t, n in cc.parse_changes(line)]
    if "v1=true" in args:  # ConfChange.AsV2: Auto with the one change
        assert len(ccs) == 1 and tr == acm.AUTO
    return tr, ccs


def walk(decode=acm.decode):
    """Every "switched to configuration" line of the fixture -> a list of
    (trace, kind, node, printed text, model text, model role, fixture leads,
    the node's changer before the change, transition, changes), kind "restore"
    or "applied", in fixture order."""
    out = []
    for name, tr in traces().items():
        st = START.get(name)
        seq = []           # the conf changes of the log, in log order
        nodes, cursor, state = {}, {}, {}
        if st:
            for i in range(1, st["nodes"] + 1):
                nodes[i] = changer_from(st["voters"], st["learners"])
                cursor[i] = 0
                state[i] = "StateLeader" if st["leader"] == i else "StateFollower"
            # what every prefix of the log leaves of the start configuration
            # (by the unbroken decode: it only places a restored node in the log)
            ref = changer_from(st["voters"], st["learners"])
            prefix = [ref.cfg.string()]
        for cmd in tr["commands"]:
            if cmd["cmd"].startswith("propose-conf-change") and not cmd["dropped"] \
                    and not cmd["ignored_cc"]:
                seq.append(proposal(cmd))
            for b in cmd["blocks"]:
                node = b["node"] if b["node"] is not None else int(cmd["cmd"].split()[1])
                if "lead_state" in b:
                    state[node] = b["lead_state"].split("State:")[1]
                for line in b.get("debug", ()):
                    m = SWITCHED.match(line)
                    if not m:
                        if "initiating automatic transition" in line:
                            seq.append((acm.AUTO, []))  # the empty change that leaves the joint
                        continue
                    nid, text = int(m.group(1)), m.group(2)
                    if b["kind"] == "recv":
                        assert any(x["type"] == "MsgSnap" for x in b.get("msgs", ())), (name, line)
                        nodes[nid] = changer_from_text(text)
                        if st:  # where the snapshot stands in the log
                            while len(prefix) <= len(seq):
                                t, ccs = seq[len(prefix) - 1]
                                assert ref.run(acm.decode(t, len(ccs)), ccs) == cc.OK
                                prefix.append(ref.cfg.string())
                            at = [k for k, p in enumerate(prefix) if p == text]
                            assert len(at) == 1, (name, line, prefix)
                            cursor[nid] = at[0]
                        out.append((name, "restore", nid, text, text, None, None, None, None, None))
                        continue
                    assert b["kind"] == "ready" and st, (name, line)
                    t, ccs = seq[cursor[nid]]
                    cursor[nid] += 1
                    before = acm.SlotChanger(S, nodes[nid].cfg.clone(),
                                             {i: p.copy() for i, p in nodes[nid].prs.items()},
                                             nodes[nid].slots)
                    model = acm.Model(1, S, decode=decode)
                    model.changers[0] = nodes[nid]
                    model.leader[0] = state.get(nid) == "StateLeader"
                    (r,) = model.apply([(0, t, len(ccs), ccs)])
                    assert r["cc_result"] == cc.OK or decode is not acm.decode, (name, line)
                    out.append((name, "applied", nid, text, nodes[nid].cfg.string(),
                                r["result"], state.get(nid) == "StateLeader", before, t, ccs))
    return out


def test_trace_pin():
    lines = walk()
    restore = [x for x in lines if x[1] == "restore"]
    applied = [x for x in lines if x[1] == "applied"]
    assert len(restore) + len(applied) == 28 and len(applied) == 21 and len(restore) == 7
    per = {}
    for name, _, nid, text, got, role, leads, *_ in applied:
        assert got == text, (name, nid)
        assert (role == acm.LEADER) == leads and role in (acm.LEADER, acm.APPLIED), (name, nid)
        per[name] = per.get(name, 0) + 1
    assert per == EXPECT
    # both roles are there.  Node 1 leads every trace but the first, and its
    # own lines are 0 + 1 + 1 + 2 + 1 + 2 + 4 of the 21
    assert sum(1 for x in applied if x[6]) == 11


def mismatches(decode):
    return [x for x in walk(decode) if x[1] == "applied" and x[3] != x[4]]


def test_control_implicit_without_autoleave():
    """JointImplicit decoded without autoLeave must not pass the pin."""
    def broken(transition, count):
        op = acm.decode(transition, count)
        return cc.OP_ENTER_JOINT if transition == acm.JOINT_IMPLICIT else op
    assert mismatches(broken)


def test_control_many_changes_as_simple():
    """count > 1 decoded as Simple must not pass the pin."""
    def broken(transition, count):
        return cc.OP_SIMPLE if count > 1 and transition == acm.AUTO else acm.decode(transition, count)
    assert mismatches(broken)


@pytest.mark.parametrize("want,code", [(acm.ANY_SLOT, cc.OK), (5, cc.OK), (1, cc.ERR_NO_SLOT),
                                       (8, cc.ERR_NO_SLOT)])
def test_named_slot(want, code):
    """A created Progress takes the named slot; a tracked one or one past S
    refuses the change and keeps the state."""
    m = acm.Model(1, S)
    m.changers[0] = changer_from((1, 2), ())
    (r,) = m.apply([(0, acm.AUTO, 1, [(cc.ADD_NODE, 9, want)])])
    assert r["cc_result"] == code
    if code == cc.OK:
        slot = 2 if want == acm.ANY_SLOT else want
        assert r["result"] == acm.APPLIED and r["new_progress"] == 1 << slot
        assert r["ids"][slot] == 9 and r["inc"] == 0b11 | 1 << slot
    else:
        assert r["result"] == acm.CHANGER_ERROR and r["tracked"] == 0b11 and r["new_progress"] == 0


def test_runs_and_refusals():
    """Rules 4 and 5 on a two-group batch: a follower applies its run, a leader
    the first record only; a refusal ends its run."""
    m = acm.Model(2, S, goff=10, max_changes=2)
    m.changers[0], m.changers[1] = changer_from((1, 2, 3), ()), changer_from((1, 2, 3), ())
    m.leader[1] = True
    add = lambda n: (acm.AUTO, 1, [(cc.ADD_NODE, n, acm.ANY_SLOT)])  # noqa: E731
    recs = [(10,) + add(4), (10, 3, 0, []), (10,) + add(5),          # APPLIED, BAD_CHANGE, SKIPPED
            (11,) + add(4), (11,) + add(5),                          # LEADER, DEFERRED
            (10,) + add(6),                                          # BAD_ORDER
            (12,) + add(4), (12,) + add(5)]                          # BAD_GROUP, SKIPPED
    res = [r["result"] for r in m.apply(recs)]
    assert res == [acm.APPLIED, acm.BAD_CHANGE, acm.SKIPPED, acm.LEADER, acm.DEFERRED,
                   acm.BAD_ORDER, acm.BAD_GROUP, acm.SKIPPED]
    assert m.changers[0].cfg.inc == {1, 2, 3, 4} and m.changers[1].cfg.inc == {1, 2, 3, 4}
    assert list(m.switched) == [0, 1]
