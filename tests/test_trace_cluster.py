"""tests/trace_cluster.py on the CPU models: the five mandatory interaction
traces (and the two add_single ones) with every role on one state and every
message built by the outbox / replies models, the coverage conditions (106
sent records, the per-type counts, run tables without slack, ALLOWED empty), negative controls that must make the
replay leave the trace at a named command line, and the oracle-level pin of
qe_become_leader on a full run table."""
import copy

import numpy as np
import pytest

from oracle import orc
from tests import trace_cluster as tc
from tests import vote_model as vm
from tests.trace_replay import traces


@pytest.fixture(scope="module")
def fixture():
    return traces()


@pytest.mark.parametrize("name", tc.TRACES)
def test_trace_replays_with_all_roles(fixture, name):
    r = tc.replay(name)
    sent, received = tc.COUNTS[name]
    assert dict(r.sent) == sent and dict(r.received) == received
    assert r.checked["records"] == sum(sent.values())  # nothing left uncompared
    assert r.checked["coalesced"] == 0
    print(f"{name}: R = {r.p.R}, {dict(r.checked)}, calls {dict(r.be.calls)}, "
          f"ALLOWED {len(tc.ALLOWED)}")


def test_coverage_conditions(fixture):
    """The mandatory set is in, the fixture's counts are the constants, the
    capacities are the fixture's, and nothing is relaxed."""
    assert set(tc.MANDATORY) <= set(tc.TRACES)
    total = 0
    for name in tc.TRACES:
        sent, received = {}, {}
        for c in fixture[name]["commands"]:
            for b in c["blocks"]:
                d = sent if b["kind"] == "ready" else received
                for m in b.get("msgs", []):
                    d[m["type"]] = d.get(m["type"], 0) + 1
        assert (sent, received) == tc.COUNTS[name], name
        assert tc.run_capacity(name, fixture[name]) == tc.RUNS[name], name
        total += sum(sent.values()) if name in tc.MANDATORY else 0
    assert total == tc.SENT_TOTAL == 106
    assert sum(len(b.get("msgs", [])) for tr in fixture.values() for c in tr["commands"]
               for b in c["blocks"] if b["kind"] == "ready") == 186
    assert tc.RUNS["campaign.txt"] == 1
    print(f"ALLOWED: {len(tc.ALLOWED)} entries")
    assert tc.ALLOWED == []


def leaves_at(name, line, **kw):
    with pytest.raises(tc.TraceMismatch) as e:
        tc.replay(name, **kw)
    assert (e.value.trace, e.value.line) == (name, line), str(e.value)
    return str(e.value)


# ---- negative controls: one broken rule each, caught at a named line ----
def test_control_reject_without_hint():
    """replies_model.build(drop_hint=True): the first rejection with a hint is
    node 3's (hint 3) in the Ready under `stabilize 2 3` (line 89), and node
    2's (hint 19) under `stabilize 1 2` (line 483)."""
    assert "hint" in leaves_at("campaign_learner_must_vote.txt", 89, drop_hint=True)
    leaves_at("probe_and_replicate.txt", 483, drop_hint=True)


def test_control_log_term_of_next_index():
    """A MsgApp whose log_term is the term of index + 1: the new leader's first
    probe (Index 4, LogTerm 1; entry 5 has term 2), line 89; Index 20, LogTerm
    6, entry 21 of term 8, line 449."""
    leaves_at("campaign_learner_must_vote.txt", 89, outbox_fault="log_term_next")
    leaves_at("probe_and_replicate.txt", 449, outbox_fault="log_term_next")


def test_control_commit_from_before_the_call():
    """Commit taken before the call: the MsgApp that announces the first commit
    (Index 3, Commit 3; 2 before the responses were stepped), `stabilize`,
    line 25."""
    assert "commit" in leaves_at("campaign.txt", 25, outbox_fault="commit_before")


def votes_whatever_the_log(node, m, *a, **kw):
    """vote_model.step without isUpToDate: the candidate's log always wins."""
    if m.type == vm.VMSG_VOTE:
        m = copy.copy(m)
        m.log_term = max(m.log_term, node.last_term() + 1)
    return vm.step(node, m, *a, **kw)


def votes_twice(node, m, *a, **kw):
    """vote_model.step that forgets the vote it cast: a second MsgVote of the
    same term is granted."""
    if m.type == vm.VMSG_VOTE and m.term == node.term:
        node = copy.deepcopy(node)
        node.vote = node.lead = vm.NONE_SLOT
    return vm.step(node, m, *a, **kw)


def test_control_vote_rule():
    """A voter that grants what the reference rejects: node 4 (log 21@6 against
    the candidate's 20@6) under `stabilize 2 3 4 5 6 7`, line 383.  The control
    "grants a second vote in a term" cannot leave any trace: no node of the
    fixture is asked twice in one term (every MsgVote arrives with a higher
    term), so `votes_twice` replays clean -- asserted here, so that a trace that
    one day holds such a request turns this into a real control."""
    leaves_at("probe_and_replicate.txt", 383, vote_step=votes_whatever_the_log)
    for name in ("campaign.txt", "campaign_learner_must_vote.txt", "probe_and_replicate.txt"):
        tc.replay(name, vote_step=votes_twice)


# ---- qe_become_leader on a full run table, at the oracle ----
def full_table(last_term, R=3):
    pb = orc.ProgressBatch(1, 3, 4, R, max_ents=0)
    md = orc.mask_dtype(3)
    pb.inc, pb.tracked = np.full(1, 7, md), np.full(1, 7, md)
    pb.self_slot = np.zeros(1, np.uint8)
    pb.lead_transferee = np.full(1, 0xFF, np.uint8)
    pb.snap_index = np.full(1, 2, np.uint64)
    for r in range(R):
        pb.run_first[r], pb.run_term[r] = 2 + 2 * r, (last_term if r == R - 1 else r + 1)
    pb.run_count[:], pb.first_index[:], pb.last_index[:] = R, 3, 2 * R + 3
    pb.committed[:] = 2 * R + 1
    return pb


def test_become_leader_on_a_full_run_table():
    """A full table whose last run has the new term: QE_BL_LEADER, run_count
    unchanged, term_start = that run's first index.  A full table whose last
    run has a lower term: QE_BL_RUNS_FULL, nothing changed."""
    pb = full_table(5)
    o = orc.become_leader(pb, np.array([5], np.uint64))
    assert int(o.result[0]) == 1
    assert int(pb.run_count[0]) == 3 and int(pb.term_start[0]) == 6
    assert int(pb.last_index[0]) == 10 and int(o.sent[0]) == 0b110
    pb = full_table(4)
    before = pb.copy()
    o = orc.become_leader(pb, np.array([5], np.uint64))
    assert int(o.result[0]) == 3 and int(o.sent[0]) == 0
    for k in ("run_count", "run_first", "run_term", "term_start", "last_index", "committed",
              "match", "next", "pw"):
        np.testing.assert_array_equal(getattr(pb, k), getattr(before, k), err_msg=k)
