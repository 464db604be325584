"""The elections of the reference's interaction traces
(tests/golden/interaction_traces.json: campaign.txt,
campaign_learner_must_vote.txt, probe_and_replicate.txt) through
tests/vote_model.py, message by message:

  - the candidate's MsgHup: the campaign's outputs against the MsgVotes of its
    Ready (term, index, logterm, the recipients);
  - every MsgVote of a "receiving messages" block on the voter: the response
    against the MsgVoteResp of the voter's next Ready (type, reject, term),
    the vote against the trace's "cast" / "rejected" line;
  - every MsgVoteResp on the candidate: the tally against the trace's "has
    received G votes and R rejections" lines, the final state against its
    "became leader at term T" line.

The voters start from the states tests/follower_traces.py derives (INITIAL);
the three candidates' states before the campaign are restated below and are
checked by the first item.  No message is skipped: the module asserts the
counts of the fixture (19 MsgVote and 18 MsgVoteResp records, each message
listed as sent and as received, four of the recorded responses rejections).
"""
import copy
import re

from tests import vote_model as vm
from tests.follower_traces import INITIAL
from tests.trace_replay import traces

TRACES = ("campaign.txt", "campaign_learner_must_vote.txt", "probe_and_replicate.txt")
S = 7  # slots: node i sits in slot i - 1
# trace -> (candidate, log after the dummy entry | "raft-log", term, lead, voters)
CANDIDATES = {
    # all three nodes sit on the snapshot (index 2, term 1)
    "campaign.txt": (1, [], 0, None, (1, 2, 3)),
    # 2 followed 1 through term 1: the empty entry 3 and the conf change 4 that
    # made the learner 3 a voter (applied on 1 and 2, lines 37-47)
    "campaign_learner_must_vote.txt": (2, [(3, 1), (4, 1)], 1, 1, (1, 2, 3)),
    # the log dumped at line 269; the last campaign before it was 5's at term 7
    "probe_and_replicate.txt": (1, "raft-log", 7, None, (1, 2, 3, 4, 5, 6, 7)),
}
VOTERS = {"campaign.txt": (1, 2, 3), "campaign_learner_must_vote.txt": (1, 2),
          "probe_and_replicate.txt": (1, 2, 3, 4, 5, 6, 7)}
COUNTS = {"MsgVote": 19, "MsgVoteResp": 18, "rejections": 4}


class Step:
    def __init__(self, trace, line, node_id, before, msg, after, out):
        self.trace, self.line, self.node_id = trace, line, node_id
        self.before, self.msg, self.after, self.out = before, msg, after, out

    @property
    def id(self):
        return f"{self.trace}:{self.line}:n{self.node_id}"


def _mask(ids):
    return sum(1 << (i - 1) for i in ids)


def response_of(out):
    """The MsgVoteResp a result stands for: (reject, term), None = silence."""
    if out["result"] == vm.VR_GRANT:
        return False, out["resp_term"]
    if out["result"] == vm.VR_REJECT:
        return True, out["resp_term"]
    return None


def replay(name, tr, steps, counts, step_fn=vm.step):
    start, dumps = None, {}
    for c in tr["commands"]:
        m = re.match(r"add-nodes \d+ .*index=(\d+)", c["cmd"])
        if m and start is None:
            start = int(m.group(1))
        m = re.match(r"raft-log (\d+)", c["cmd"])
        if m:
            dumps[int(m.group(1))] = [(i, t) for t, i in c["log"]]
    cand_id, clog, cterm, clead, cvoters = CANDIDATES[name]

    def make(n, log, commit, term, lead, voters):
        if log is None:
            ents = [(0, 0)]
        else:
            ents = [(start, 1)] + (dumps[n] if log == "raft-log" else list(log))
        return vm.Node(ents, inc=_mask(voters), tracked=_mask(range(1, 8)), self_slot=n - 1,
                       committed=commit if commit is not None else ents[0][0], term=term,
                       lead=vm.NONE_SLOT if lead is None else lead - 1)

    nodes, owed = {}, {}

    def voter(n):
        if n not in nodes:
            log, commit, term, lead = INITIAL.get(name, {}).get(n, (None, 0, 0, None))
            nodes[n] = make(n, log, commit, term, lead, VOTERS[name])
        return nodes[n]

    def run(n, line, msg):
        before = nodes[n]
        after, out = step_fn(before, msg, 0, S, 10)
        steps.append(Step(name, line, n, copy.deepcopy(before), msg, after, out))
        nodes[n] = after
        return out

    won = False
    for c in tr["commands"]:
        for b in c["blocks"]:
            n = b["node"] if b["node"] is not None else int(c["cmd"].split()[1])
            votes = [m for m in b.get("msgs", []) if m["type"] == "MsgVote"]
            resps = [m for m in b.get("msgs", []) if m["type"] == "MsgVoteResp"]
            where = (name, c["line"], n)
            if b["kind"] == "ready" and votes:
                # the campaign that sent them
                assert n == cand_id and n not in nodes, where
                nodes[n] = make(n, clog, None, cterm, clead, cvoters)
                out = run(n, c["line"], vm.Msg(vm.VMSG_HUP))
                assert out["result"] == vm.VR_CAMPAIGN_VOTE, where
                assert "StateCandidate" in b["lead_state"] and b["term"] == nodes[n].term, where
                for m in votes:
                    counts["MsgVote"] += 1
                    assert (m["term"], m["index"], m["logterm"]) == (
                        out["resp_term"], nodes[n].last_index(), out["req_log_term"]), (where, m)
                assert _mask(m["to"] for m in votes) == out["req_to"], where
            elif b["kind"] == "ready" and resps:
                for m in resps:
                    counts["MsgVoteResp"] += 1
                    counts["rejections"] += int(m["reject"])
                    assert response_of(owed[n].pop(0)) == (m["reject"], m["term"]), (where, m)
                assert not owed[n], where
                assert b["term"] == nodes[n].term, where
            elif b["kind"] == "recv" and votes:
                v = voter(n)
                for m in votes:
                    counts["MsgVote"] += 1
                    for d in b["debug"]:  # the term the trace reports before the message
                        t = re.match(rf"INFO {n} \[term: (\d+)\] received", d)
                        if t and int(t.group(1)) != v.term:
                            v = nodes[n] = copy.deepcopy(v)
                            v.term = int(t.group(1))
                    line = [d for d in b["debug"] if "cast MsgVote" in d or "rejected MsgVote" in d][0]
                    lt, li = map(int, re.search(r"\[logterm: (\d+), index: (\d+), vote", line).groups())
                    assert (lt, li) == (v.last_term(), v.last_index()), (where, line)
                    out = run(n, c["line"], vm.Msg(vm.VMSG_VOTE, m["from"] - 1, m["term"], m["index"],
                                                   m["logterm"]))
                    owed.setdefault(n, []).append(out)
                    cast = "cast MsgVote" in line
                    assert cast == (out["result"] == vm.VR_GRANT), (where, line)
                    assert nodes[n].vote == (m["from"] - 1 if cast else vm.NONE_SLOT), where
                    assert any(f"became follower at term {m['term']}" in d for d in b["debug"]) == (
                        out["events"] == vm.TEV_RESET), where
            elif b["kind"] == "recv" and resps:
                assert n == cand_id, where
                tallies = [tuple(map(int, re.search(r"received (\d+) MsgVoteResp votes and (\d+) vote",
                                                    d).groups()))
                           for d in b["debug"] if "has received" in d]
                for m in resps:
                    counts["MsgVoteResp"] += 1
                    counts["rejections"] += int(m["reject"])
                    was = nodes[n].state
                    out = run(n, c["line"], vm.Msg(vm.VMSG_VOTE_RESP, m["from"] - 1, m["term"],
                                                   flags=vm.VMF_REJECT if m["reject"] else 0))
                    if was == vm.ST_CANDIDATE:
                        g, r = tallies.pop(0)
                        if out["result"] == vm.VR_PENDING:
                            node = nodes[n]
                            assert (g, r) == (bin(node.granted).count("1"),
                                              bin(node.voted & ~node.granted).count("1")), (where, m)
                        else:
                            assert out["result"] == vm.VR_WON and out["elected"] == 1, (where, m)
                    else:  # a response that arrives after the election
                        assert was == vm.ST_LEADER and out["result"] == vm.VR_IGNORED, (where, m)
                assert not tallies, where
                term = [int(re.search(r"became leader at term (\d+)", d).group(1))
                        for d in b["debug"] if "became leader" in d]
                assert term, where
                node = nodes[n]
                assert (node.state, node.term, node.lead) == (vm.ST_LEADER, term[0], n - 1), where
                won = True
    assert won and not any(owed.values()), name


def replay_all(step_fn=vm.step):
    """-> (steps, counts); raises where the model and a trace disagree."""
    steps = []
    counts = {"MsgVote": 0, "MsgVoteResp": 0, "rejections": 0, "skipped": 0}
    all_traces = traces()
    for name in TRACES:
        replay(name, all_traces[name], steps, counts, step_fn)
    assert counts == dict(COUNTS, skipped=0), counts
    return steps, counts


if __name__ == "__main__":
    steps, counts = replay_all()
    print(f"{len(steps)} steps; {counts}")
