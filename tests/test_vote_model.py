"""tests/vote_model.py against the reference's own expectations: the vote
tables of tests/golden/vote_tables.json (the reference's table tests restated
per message), the elections of the interaction traces (tests/vote_traces.py),
negative controls that prove the comparisons bite, and the safety properties
of a vote over random states and messages."""
import copy
import json
import os

import numpy as np
import pytest

from tests import vote_model as vm
from tests import vote_traces as vt

HERE = os.path.dirname(os.path.abspath(__file__))
RESP_TYPE = {vm.VMSG_VOTE: "MsgVoteResp", vm.VMSG_PREVOTE: "MsgPreVoteResp"}


def tables():
    with open(os.path.join(HERE, "golden", "vote_tables.json")) as f:
        return json.load(f)


def _node(d):
    ents = [(0, 0)] + [(i, t) for i, t in d["log"]]
    return vm.Node(ents, elapsed=d["elapsed"], inc=d["inc"], tracked=d["tracked"],
                   self_slot=d["self_slot"], term=d["term"], state=d["state"], lead=d["lead"],
                   vote=d["vote"])


def _msg(d):
    return vm.Msg(d["type"], d["from"], d["term"], d["index"], d["log_term"], d["flags"])


def fixture_cases():
    """-> [(id, S, flags, election_timeout, node, msg, want)], every single-message row."""
    out = []
    for name, t in tables().items():
        for k, c in enumerate(t.get("cases", [])):
            out.append((f"{name}#{k}", t["num_slots"], t["flags"], t.get("election_timeout", 10),
                        _node(c["node"]), _msg(c["msg"]), c["want"]))
    return out


def check_case(S, flags, et, node, msg, want, step_fn=vm.step):
    after, out = step_fn(node, msg, flags, S, et)
    resp = vt.response_of(out)
    if want["response"] is None:
        assert resp is None, out
        assert out["result"] == vm.VR_IN_LEASE, out
    else:
        assert resp is not None, out
        assert want["response"]["type"] == RESP_TYPE[msg.type]
        assert resp[0] == want["response"]["reject"], out
        if "term" in want["response"]:
            assert resp[1] == want["response"]["term"], out
    for k in ("term", "vote", "state"):
        if k in want:
            assert getattr(after, k) == want[k], (k, getattr(after, k))
    if "vote_in" in want:
        assert after.vote in want["vote_in"]
    return after, out


def test_table_counts():
    t = tables()
    assert len(t["TestRecvMsgVote"]["cases"]) == len(t["TestRecvMsgPreVote"]["cases"]) == 21
    assert len(t["TestVoteFromAnyState"]["cases"]) == len(t["TestPreVoteFromAnyState"]["cases"]) == 4
    assert (len(t["TestFollowerVote"]["cases"]), len(t["TestVoter"]["cases"])) == (6, 9)
    assert len(t["TestLeaderElectionInOneRoundRPC"]["sequences"]) == 13
    assert len(fixture_cases()) == 74


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_tables(case):
    check_case(*case[1:])


def run_sequence(t, seq, step_fn=vm.step):
    """MsgHup, then the responses at the candidate's term -> (node, results)."""
    S = t["num_slots"]
    node, out = step_fn(_node(seq["node"]), vm.Msg(vm.VMSG_HUP), t["flags"], S, 10)
    results = [out["result"]]
    for r in seq["responses"]:
        m = vm.Msg(vm.VMSG_VOTE_RESP, r["from"], node.term, flags=vm.VMF_REJECT if r["reject"] else 0)
        node, out = step_fn(node, m, t["flags"], S, 10)
        results.append(out["result"])
    return node, results


def test_election_in_one_round():
    t = tables()["TestLeaderElectionInOneRoundRPC"]
    for k, seq in enumerate(t["sequences"]):
        node, results = run_sequence(t, seq)
        assert (node.state, node.term) == (seq["want"]["state"], seq["want"]["term"]), (k, results)
        assert (vm.VR_WON in results) == (node.state == vm.ST_LEADER), k
        assert (vm.VR_LOST in results) == (node.state == vm.ST_FOLLOWER), k


def test_traces():
    steps, counts = vt.replay_all()
    assert counts == {"MsgVote": 19, "MsgVoteResp": 18, "rejections": 4, "skipped": 0}
    assert len(steps) == 21  # 3 campaigns, 9 requests received, 9 responses received
    print(counts)


# ---- negative controls: each comparison fails when its subject is changed ----
def test_control_changed_reject_flag():
    for case in fixture_cases():
        want = copy.deepcopy(case[6])
        if want["response"] is None:
            continue
        want["response"]["reject"] = not want["response"]["reject"]
        with pytest.raises(AssertionError):
            check_case(*case[1:6], want)


def test_control_changed_response_term():
    def wrong_term(node, m, *a, **kw):
        after, out = vm.step(node, m, *a, **kw)
        if out["result"] in (vm.VR_GRANT, vm.VR_REJECT):
            out = dict(out, resp_term=out["resp_term"] + 1)
        return after, out

    with pytest.raises(AssertionError):
        vt.replay_all(wrong_term)
    rows = [c for c in fixture_cases() if c[6]["response"] and "term" in c[6]["response"]]
    assert len(rows) >= 9
    for case in rows:
        with pytest.raises(AssertionError):
            check_case(*case[1:], step_fn=wrong_term)


def test_control_lease_row_without_check_quorum():
    rows = [c for c in fixture_cases() if c[6]["response"] is None]
    assert len(rows) == 6
    for cid, S, flags, et, node, msg, want in rows:
        assert flags & vm.VOTE_CHECK_QUORUM
        with pytest.raises(AssertionError):
            check_case(S, 0, et, node, msg, want)


def test_control_wrong_tally():
    """A model that forgets that the first vote sticks fails the traces' tallies
    or the one-round table."""
    def forgetful(node, m, *a, **kw):
        if m.type == vm.VMSG_VOTE_RESP and node.state == vm.ST_CANDIDATE:
            node = copy.deepcopy(node)
            node.granted &= 1 << node.self_slot
        return vm.step(node, m, *a, **kw)

    t = tables()["TestLeaderElectionInOneRoundRPC"]
    bad = 0
    for seq in t["sequences"]:
        node, _ = run_sequence(t, seq, forgetful)
        bad += node.state != seq["want"]["state"]
    assert bad > 0
    with pytest.raises(AssertionError):
        vt.replay_all(forgetful)


# ---- properties ----
def test_properties_over_random_pairs():
    """20 000 (node, message) pairs: 2 500 random nodes, 8 consecutive messages
    each, every flag combination and mask form."""
    rng = np.random.default_rng(20240)
    pairs, seen = 0, set()
    for k in range(2500):
        S = (3, 5, 9)[k % 3]
        flags, masks, cand = k % 4, ("none", "inc", "joint")[(k // 4) % 3], (k // 12) % 4 != 0
        node = vm.gen_node(rng, (1, 4, 16)[(k // 3) % 3], S, masks)
        real_votes = {}  # term -> the candidate that got this node's vote
        if node.vote < S:
            real_votes[node.term] = node.vote
        for _ in range(8):
            m = vm.gen_msg(rng, node, S)
            snapshot = copy.deepcopy(node)
            after, out = vm.step(node, m, flags, S, 10, cand)
            pairs += 1
            seen.add(out["result"])
            assert node.key() == snapshot.key()  # the input is never mutated
            assert after.term >= node.term
            if m.type == vm.VMSG_PREVOTE:
                assert (after.term, after.vote) == (node.term, node.vote), m
                assert after is node
            if out["result"] >= vm.VR_REFUSED or out["result"] in (vm.VR_NONE, vm.VR_IN_LEASE):
                assert after is node
                assert out["events"] == 0 and out["elected"] == 0
            if out["result"] == vm.VR_GRANT and m.type == vm.VMSG_VOTE:
                assert after.term == m.term == out["resp_term"]
                assert real_votes.setdefault(after.term, m.frm) == m.frm, (real_votes, m)
            if after.vote != node.vote and after.vote < S:
                # (its own campaign is a real vote too)
                assert real_votes.setdefault(after.term, after.vote) == after.vote
            assert (out["elected"] == 1) == (out["result"] == vm.VR_WON)
            assert ("resp_term" in out) == (out["result"] in (vm.VR_GRANT, vm.VR_REJECT,
                                                               vm.VR_CAMPAIGN_PREVOTE,
                                                               vm.VR_CAMPAIGN_VOTE))
            assert ("req_to" in out) == ("req_log_term" in out) == (
                out["result"] in (vm.VR_CAMPAIGN_PREVOTE, vm.VR_CAMPAIGN_VOTE))
            node = after
    assert pairs == 20000
    assert seen == vm.ALL_RESULTS, sorted(vm.VR_NAMES[c] for c in vm.ALL_RESULTS - seen)


def test_generated_nodes_keep_the_last_run_invariant():
    rng = np.random.default_rng(3)
    for R in (1, 4, 16):
        for _ in range(300):
            n = vm.gen_node(rng, R, 5)
            assert n.runs[-1][0] <= n.last_index() and n.runs[-1][1] == n.last_term()


@pytest.mark.parametrize("case", vm.RUN_CASES, ids=str)
def test_every_result_code_appears(case):
    """The generator of the GPU differential is proven here, from the model's
    outcomes: a full launch meets every result code its flags allow, a launch
    without the Votes rows or self_slot every code it can reach."""
    S, R, masks, flags, cand, have_self = case
    seen = vm.random_run(case)
    if cand and have_self:
        want = set(vm.ALL_RESULTS)
        if not flags & vm.VOTE_CHECK_QUORUM:
            want.discard(vm.VR_IN_LEASE)
        if not flags & vm.VOTE_PREVOTE:
            want.discard(vm.VR_CAMPAIGN_PREVOTE)
    else:
        want = {vm.VR_NONE, vm.VR_IGNORED, vm.VR_GRANT, vm.VR_REJECT, vm.VR_BAD_MSG}
        want |= {vm.VR_IN_LEASE} if flags & vm.VOTE_CHECK_QUORUM else set()
    assert want <= seen, sorted(vm.VR_NAMES[c] for c in want - seen)


def test_the_random_run_meets_every_result_code():
    full = [c for c in vm.RUN_CASES if c[4] and c[5] and c[3] == 3]
    assert full and all(vm.random_run(c) == vm.ALL_RESULTS for c in full)
