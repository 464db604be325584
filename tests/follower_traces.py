"""The reference's interaction traces (tests/golden/interaction_traces.json)
from the receivers' side: every MsgApp and MsgHeartbeat of a "receiving
messages" block stepped through tests/follower_model.py, the response
compared with the MsgAppResp / MsgHeartbeatResp of the node's next Ready
(index, reject, hint, logterm), the node's term / commit / entries with that
Ready's HardState and entry lists where the trace prints them.

A receiver's state before its first recorded message is restated from the
trace itself: the `raft-log` dumps, the snapshot `add-nodes ... index=N`
starts every node from (term 1, interaction_env_handler_add_nodes.go:91), the
"[term: T] received" and "restored snapshot [index: I, term: T]" lines, the
HardState of the Ready that precedes the message, and -- where a part of the
trace ran with the log switched off -- the entries its leader appended in
that part (INITIAL below says which).  Messages the follower entry point
does not take (MsgVote, MsgSnap, ...) are applied as the trace reports them.
"""
import copy
import re

from tests import follower_model as fm
from tests.trace_replay import traces

# node -> (log after the dummy entry | "raft-log", commit | None = the first
# HardState line, term, lead); nodes not listed start empty (add-nodes without
# index: dummy (0, 0), term 0), nodes that only lead are not followed.
INITIAL = {
    # the seven logs are dumped at lines 269-340; `campaign 1` follows
    "probe_and_replicate.txt": {n: ("raft-log", None, 0, None) for n in range(2, 8)},
    # line 24 `stabilize` (log off): 2 got the leader's empty entry 11 and its commit
    "snapshot_succeed_via_app_resp.txt": {2: ([(11, 1)], 11, 1, 1)},
    # the election itself is printed: both voters still sit on the snapshot
    "campaign.txt": {2: ([], 2, 0, None), 3: ([], 2, 0, None)},
    # line 26 `stabilize` (log off): the learner got entry 3 of term 1 and its
    # commit; the conf change after it went to 1 and 2 only (lines 37, 43)
    "campaign_learner_must_vote.txt": {3: ([(3, 1)], 3, 1, 1)},
    # line 16 `stabilize` (log off): both followers hold the leader's entry 3
    "confchange_v1_remove_leader.txt": {2: ([(3, 1)], 3, 1, 1), 3: ([(3, 1)], 3, 1, 1)},
}
# (trace, line, reason): messages whose receiver's prior log the fixture does
# not determine.  None is needed.
SKIP = []
MAX_SKIP = 8


class Step:
    def __init__(self, trace, line, node_id, before, msg, after, out):
        self.trace, self.line, self.node_id = trace, line, node_id
        self.before, self.msg, self.after, self.out = before, msg, after, out

    @property
    def id(self):
        return f"{self.trace}:{self.line}:n{self.node_id}"


def _msg(m):
    ents = [(i, t) for t, i in m["entries"]]
    assert [i for i, _ in ents] == list(range(m["index"] + 1, m["index"] + 1 + len(ents)))
    runs = []
    for _, t in ents:
        if runs and runs[-1][1] == t:
            runs[-1][0] += 1
        else:
            runs.append([1, t])
    ty = fm.LMSG_APP if m["type"] == "MsgApp" else fm.LMSG_HEARTBEAT
    return fm.Msg(ty, m["from"] - 1, m["term"], m["index"], m["logterm"], m["commit"], runs)


class _Follower:
    """A node of a trace as its Readies show it."""

    def __init__(self, node, commit_known):
        self.node, self.commit_known = node, commit_known
        self.applied = node.committed if commit_known else None
        self.unstable = None  # first index appended since the last Ready
        self.resps = []       # responses owed to the next Ready


def replay(name, tr, steps, skipped):
    start = None
    dumps = {}
    for c in tr["commands"]:
        m = re.match(r"add-nodes \d+ .*index=(\d+)", c["cmd"])
        if m and start is None:
            start = int(m.group(1))
        m = re.match(r"raft-log (\d+)", c["cmd"])
        if m:
            dumps[int(m.group(1))] = [(i, t) for t, i in c["log"]]
    fols = {}

    def follower(n):
        if n not in fols:
            log, commit, term, lead = INITIAL.get(name, {}).get(n, (None, 0, 0, None))
            if log is None:  # a node added empty
                ents = [(0, 0)]
            else:
                ents = [(start, 1)] + (dumps[n] if log == "raft-log" else log)
            node = fm.Node(ents, committed=commit if commit is not None else ents[0][0], term=term,
                           lead=fm.NONE_SLOT if lead is None else lead - 1)
            fols[n] = _Follower(node, commit is not None)
        return fols[n]

    # the nodes to follow: whoever is sent a MsgApp, a MsgHeartbeat or a MsgSnap
    receivers = {b["node"] for c in tr["commands"] for b in c["blocks"] if b["kind"] == "recv"
                 for m in b["msgs"] if m["type"] in ("MsgApp", "MsgHeartbeat", "MsgSnap")}
    for c in tr["commands"]:
        for b in c["blocks"]:
            n = b["node"]
            if n not in receivers or b["kind"] == "status":
                continue
            assert "StateLeader" not in b.get("lead_state", ""), (name, c["line"], n)
            if b["kind"] == "recv":
                f = follower(n)
                for m in b["msgs"]:
                    if m["type"] in ("MsgApp", "MsgHeartbeat"):
                        if (name, c["line"]) in [(s[0], s[1]) for s in SKIP]:
                            skipped.append((name, c["line"], n))
                            continue
                        assert f.commit_known, (name, c["line"], n)
                        msg, before = _msg(m), f.node
                        after, out = fm.step(before, msg, 0, 16, 16)
                        steps.append(Step(name, c["line"], n, copy.deepcopy(before), msg, after, out))
                        f.node = after
                        f.resps.append((m["type"], out))
                        ci = out.get("append_from", 0)
                        if ci:
                            f.unstable = ci if f.unstable is None else min(f.unstable, ci)
                    elif m["type"] == "MsgSnap":
                        line = [d for d in b["debug"] if "restored snapshot" in d][0]
                        idx, term = map(int, re.search(r"\[index: (\d+), term: (\d+)\]", line).groups())
                        assert idx == m["snap_index"]
                        f.node = fm.Node([(idx, term)], committed=idx, term=max(f.node.term, m["term"]),
                                         lead=m["from"] - 1)
                        f.applied, f.unstable, f.commit_known = idx, None, True
                        f.resps.append(("MsgSnap", {"resp_index": idx}))
                    else:
                        # the term preamble for a message the entry point does not take
                        for d in b["debug"]:
                            t = re.match(rf"INFO {n} \[term: (\d+)\] received", d)
                            if t:
                                f.node.term = int(t.group(1))
                        if m["term"] > f.node.term:
                            assert any(f"became follower at term {m['term']}" in d for d in b["debug"])
                            f.node = copy.deepcopy(f.node)
                            f.node.become_follower(m["term"], fm.NONE_SLOT)
            else:  # this node's Ready
                if n not in fols:
                    continue
                f = fols[n]
                for m in b["msgs"]:
                    if m["type"] not in ("MsgAppResp", "MsgHeartbeatResp"):
                        continue
                    kind, out = f.resps.pop(0)
                    where = (name, c["line"], n, m)
                    if kind == "MsgHeartbeat":
                        assert m["type"] == "MsgHeartbeatResp", where
                        assert out["result"] == fm.FR_HEARTBEAT_RESP, where
                        continue
                    assert m["type"] == "MsgAppResp", where
                    rej = out.get("result") == fm.FR_APP_REJECT
                    assert (m["index"], m["reject"]) == (out["resp_index"], rej), where
                    # an accepted response carries neither field (zero)
                    assert m["hint"] == out.get("reject_hint", 0), where
                    assert m["logterm"] == out.get("resp_log_term", 0), where
                assert not f.resps, (name, c["line"], n)
                if "term" in b:
                    assert b["term"] == f.node.term, (name, c["line"], n)
                if "commit" in b:
                    if not f.commit_known:  # the HardState line that restates it
                        f.node = copy.deepcopy(f.node)
                        f.node.committed = f.applied = b["commit"]
                        f.commit_known = True
                    assert b["commit"] == f.node.committed, (name, c["line"], n)
                if f.commit_known:
                    # Entries (appended since the last Ready), then CommittedEntries
                    node, dummy = f.node, f.node.ents[0][0]
                    want = [] if f.unstable is None else node.ents[f.unstable - dummy:]
                    want = want + node.ents[f.applied + 1 - dummy: node.committed + 1 - dummy]
                    got = [(i, t) for t, i in b.get("entries", [])]
                    assert got == want, (name, c["line"], n)
                if f.commit_known:
                    f.applied, f.unstable = f.node.committed, None
    for n, f in fols.items():
        assert not f.resps, (name, n)


def replay_all():
    """-> (steps, skipped)"""
    steps, skipped = [], []
    for name, tr in traces().items():
        replay(name, tr, steps, skipped)
    return steps, skipped
