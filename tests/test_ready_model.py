"""qe_ready_note / qe_ready / qe_advance on the CPU: the golden Ready blocks the
reference printed (tests/golden/ready_blocks.json, totals asserted), the rules'
sequential restatement (tests/ready_model.py) on hand cases -- each arm of
truncateAndAppend, restore, stableTo with a changed term, appliedTo out of
range, an empty HardState that is not listed, E cutting the entries, max_apply
cutting the apply range -- and the all-roles trace replay with every Ready
field taken from the records (tests/ready_sim.py): all 72 blocks of the five
mandatory traces, and three negative controls that must leave a trace."""
import numpy as np
import pytest

from tests import ready_model as rdm
from tests import ready_sim as rsim
from tests import trace_cluster as tc
from tests.golden import make_ready_golden as mrg

NONE = rdm.NONE


@pytest.fixture(scope="module")
def blocks():
    return rsim.ready_blocks()


def test_golden_totals(blocks):
    """What the extractor counted in raft/testdata: 138 Ready blocks, 58 with
    MustSync=true, 7 with a Snapshot; 31 SoftState and 66 HardState lines; 39
    blocks with Entries (75 entries), 40 with CommittedEntries (74)."""
    assert len(blocks) == 10
    assert mrg.totals(blocks) == mrg.TOTALS
    assert mrg.TOTALS["blocks"] == 138 and mrg.TOTALS["must_sync"] == 58
    assert mrg.TOTALS["snapshot"] == 7
    assert {k: len(blocks[k]) for k in rsim.BLOCKS} == rsim.BLOCKS
    for bs in blocks.values():
        assert [b["line"] for b in bs] == sorted(b["line"] for b in bs)
        for b in bs:
            assert set(b) == {"line", "cmd_line", "node", "must_sync", "soft", "hard", "entries",
                              "committed", "snapshot"}


def test_golden_parser_on_both_block_forms():
    """An unindented process-ready block and an indented stabilize block."""
    text = """process-ready 2
----
Ready MustSync=true:
Lead:0 State:StateCandidate
HardState Term:2 Vote:2 Commit:4
Messages:
2->1 MsgVote Term:2 Log:1/4

stabilize 3
----
> 3 receiving messages
  1->3 MsgApp Term:1 Log:1/3 Commit:3 Entries:[1/4 EntryNormal ""]
> 3 handling Ready
  Ready MustSync=true:
  HardState Term:1 Commit:4
  Entries:
  1/4 EntryNormal ""
  Snapshot Index:3 Term:1 ConfState:Voters:[1 2 3]
  CommittedEntries:
  1/4 EntryNormal ""
  Messages:
  3->1 MsgAppResp Term:1 Log:0/4
"""
    a, b = mrg.parse_file(text.split("\n"))
    assert a == dict(line=3, cmd_line=1, node=2, must_sync=True, soft="Lead:0 State:StateCandidate",
                     hard=[2, 2, 4], entries=[], committed=[], snapshot=None)
    assert b == dict(line=14, cmd_line=9, node=3, must_sync=True, soft=None, hard=[1, 0, 4],
                     entries=[[1, 4]], committed=[[1, 4]], snapshot=3)


# ---- hand cases ----
def one(runs, last, committed, term=3, vote=NONE, lead=1, state=0, S=3, goff=0):
    """One group: its log as term runs [(first, term), ...] (run 0 the dummy)."""
    R = len(runs)
    st = rdm.state(num_groups=1, group_offset=goff, num_slots=S, stride=1, log_runs=R,
                   committed=[committed], last_index=[last], run_first=[f for f, _ in runs],
                   run_term=[t for _, t in runs], run_count=[R], term=[term], state=[state],
                   lead=[lead], vote=[vote])
    rs = rsim.fresh_rows(1)
    rdm.reset(st, rs)
    rs.applied[0] = committed
    return st, rs


def test_note_truncate_and_append_arms():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5)
    rs.stable[0] = 7  # unstable.offset 8, entries 8..10
    # after == offset + len: a plain append, the offset stays
    rdm.note(st, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[11])
    assert rs.stable[0] == 7
    # offset < after: truncate inside the unstable part, the offset stays
    rdm.note(st, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[9])
    assert rs.stable[0] == 7
    # after == offset: replaced from the offset on, the offset stays
    rdm.note(st, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[8])
    assert rs.stable[0] == 7
    # after < offset: the stable part is truncated, offset = after
    rdm.note(st, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[6])
    assert rs.stable[0] == 5
    # nothing appended (append_from 0), and every other result: no move
    rdm.note(st, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[0])
    rdm.note(st, rs, follow_result=[5], append_from=[2])
    assert rs.stable[0] == 5 and rs.snap_pending[0] == 0


def test_note_restore():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5)
    rdm.note(st, rs, snap_result=[4], snap_resp_index=[40])  # FAST_FORWARD: no restore
    assert (rs.stable[0], rs.snap_pending[0]) == (10, 0)
    rdm.note(st, rs, snap_result=[rdm.SR_RESTORED], snap_resp_index=[40])
    assert (rs.stable[0], rs.snap_pending[0]) == (40, 40)
    st, rs2 = one([(40, 2)], last=40, committed=40, term=2)
    rs2.stable[0], rs2.snap_pending[0], rs2.applied[0] = 40, 40, 5
    (rec,), _ = rdm.ready(st, rs2)
    assert rec["flags"] & rdm.SNAP and rec["snap_index"] == 40
    assert rec["ent_count"] == rec["apply_count"] == 0  # nothing after the snapshot
    assert rdm.advance(st, rs2, [rec]) == [rdm.ADV_OK]
    assert (rs2.applied[0], rs2.snap_pending[0]) == (40, 0)
    assert rdm.ready(st, rs2)[0] == []


def test_nothing_changed_is_not_listed_and_pending_lists_it():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5)
    assert rdm.ready(st, rs)[0] == []
    (rec,), stats = rdm.ready(st, rs, pending=[1])
    assert rec["flags"] == 0 and rec["ent_first"] == 11 and stats[rdm.STAT_GROUPS] == 1


def test_empty_hard_state_is_not_listed():
    """term 0, no vote, commit 0 against a prev that differs: hard_changed, but
    IsEmptyHardState -- HasReady says no."""
    st, rs = one([(0, 0)], last=0, committed=0, term=0, lead=NONE)
    rs.prev_term[0], rs.prev_commit[0], rs.prev_vote[0] = 4, 2, 1
    assert rdm.ready(st, rs)[0] == []
    (rec,), _ = rdm.ready(st, rs, pending=[1])
    assert not rec["flags"] & rdm.HARD
    assert rec["flags"] & rdm.MUST_SYNC  # MustSync compares term and vote all the same
    # two encodings of None are one value
    st, rs = one([(0, 0), (1, 1)], last=3, committed=3, vote=0xFF, lead=0x7F)
    rs.prev_vote[0], rs.prev_lead[0] = 0x33, 0xFF
    assert rdm.ready(st, rs)[0] == []


def test_hard_and_soft_deltas_and_must_sync():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5, vote=2)
    rs.prev_commit[0] = 4
    (rec,), _ = rdm.ready(st, rs)
    assert rec["flags"] == rdm.HARD  # a commit change alone: no MustSync
    rs.prev_vote[0] = NONE
    (rec,), _ = rdm.ready(st, rs)
    assert rec["flags"] == rdm.HARD | rdm.MUST_SYNC and rec["vote"] == 2
    rs.prev_state[0] = 1
    (rec,), _ = rdm.ready(st, rs)
    assert rec["flags"] == rdm.HARD | rdm.MUST_SYNC | rdm.SOFT
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK]
    assert (rs.prev_term[0], rs.prev_commit[0], rs.prev_vote[0]) == (3, 5, 2)
    assert (rs.prev_lead[0], rs.prev_state[0]) == (1, 0)
    assert rdm.ready(st, rs)[0] == []


def test_entries_cut_by_runs():
    runs = [(2, 1), (3, 2), (5, 3), (6, 5), (9, 7)]
    st, rs = one(runs, last=12, committed=4, term=7)
    rs.stable[0] = 3
    (rec,), _ = rdm.ready(st, rs, ent_runs=0)
    assert (rec["ent_first"], rec["ent_count"], rec["ent_last_term"]) == (4, 9, 7)
    assert rec["ents"] == [] and rec["flags"] == rdm.MUST_SYNC
    (rec,), _ = rdm.ready(st, rs, ent_runs=4)
    assert rec["ents"] == [(1, 2), (1, 3), (3, 5), (4, 7)] and not rec["flags"] & rdm.ENTS_CUT
    (rec,), _ = rdm.ready(st, rs, ent_runs=2)
    assert rec["ents"] == [(1, 2), (1, 3)] and rec["flags"] & rdm.ENTS_CUT
    assert (rec["ent_count"], rec["ent_last_term"]) == (2, 3)
    assert rdm.expand(rec["ent_first"], rec["ents"]) == [[2, 4], [3, 5]]
    # the advance moves stable to where the list ended; the next Ready lists the rest
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK] and rs.stable[0] == 5
    (rec,), _ = rdm.ready(st, rs, ent_runs=2)
    assert rec["ents"] == [(3, 5), (4, 7)] and not rec["flags"] & rdm.ENTS_CUT
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK] and rs.stable[0] == 12
    assert rdm.ready(st, rs)[0] == []


def test_apply_range_and_max_apply():
    runs = [(2, 1), (3, 2), (6, 5)]
    st, rs = one(runs, last=12, committed=10, term=5)
    rs.applied[0], rs.prev_commit[0] = 0, 10  # below the dummy: off = run_first[0] + 1
    (rec,), _ = rdm.ready(st, rs, ent_runs=4)
    assert (rec["apply_first"], rec["apply_count"]) == (3, 8)
    assert rec["apply"] == [(3, 2), (5, 5)] and rec["flags"] == 0
    (rec,), _ = rdm.ready(st, rs, ent_runs=4, max_apply=4)
    assert rec["apply"] == [(3, 2), (1, 5)] and rec["flags"] == rdm.APPLY_CUT
    (rec,), _ = rdm.ready(st, rs, ent_runs=0, max_apply=4)
    assert (rec["apply_first"], rec["apply_count"], rec["apply"]) == (3, 4, [])
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK] and rs.applied[0] == 6
    (rec,), _ = rdm.ready(st, rs, ent_runs=1)  # E cuts the apply list too
    assert rec["apply"] == [(4, 5)] and (rec["apply_first"], rec["apply_count"]) == (7, 4)
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK] and rs.applied[0] == 10
    assert rdm.ready(st, rs)[0] == []
    rs.applied[0] = 11  # past committed: nothing to apply
    assert rdm.ready(st, rs)[0] == []


def test_stable_to_with_a_changed_term():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5, term=1)
    rs.stable[0] = 7
    (rec,), _ = rdm.ready(st, rs, ent_runs=4)
    assert rec["ents"] == [(3, 1)] and rec["ent_last_term"] == 1
    # the log is truncated and rewritten under the Ready: 9.. now of term 2
    st2, _ = one([(0, 0), (1, 1), (9, 2)], last=10, committed=5, term=2)
    rdm.note(st2, rs, follow_result=[rdm.FR_APP_ACCEPT], append_from=[9])
    assert rs.stable[0] == 7
    assert rdm.advance(st2, rs, [rec]) == [rdm.ADV_OK_STALE_ENTRIES] and rs.stable[0] == 7
    (rec2,), _ = rdm.ready(st2, rs, ent_runs=4)
    assert rec2["ents"] == [(1, 1), (2, 2)]  # listed again
    # a record whose last entry is past the log
    st3, _ = one([(0, 0), (1, 1)], last=8, committed=5, term=1)
    assert rdm.advance(st3, rs, [rec]) == [rdm.ADV_OK_STALE_ENTRIES] and rs.stable[0] == 7
    assert rdm.advance(st2, rs, [rec2]) == [rdm.ADV_OK] and rs.stable[0] == 10


def test_applied_to_out_of_range_and_bad_group():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=5, goff=1 << 33)
    rs.applied[0], rs.prev_commit[0] = 3, 4
    (rec,), _ = rdm.ready(st, rs)
    assert (rec["apply_first"], rec["apply_count"]) == (4, 2)
    before = {k: np.array(getattr(rs, k)) for k in rdm.STATE_ROWS}
    past = dict(rec, apply_count=3)            # committed < newApplied
    below = dict(rec, apply_first=1, apply_count=2)  # newApplied < applied
    stray = dict(rec, group=rec["group"] + 1)
    low = dict(rec, group=(1 << 33) - 1)
    assert rdm.advance(st, rs, [past, below, stray, low]) == [
        rdm.ADV_APPLIED_RANGE, rdm.ADV_APPLIED_RANGE, rdm.ADV_BAD_GROUP, rdm.ADV_BAD_GROUP]
    for k, v in before.items():
        np.testing.assert_array_equal(getattr(rs, k), v, err_msg=k)
    assert rdm.advance(st, rs, [rec]) == [rdm.ADV_OK] and rs.applied[0] == 5


def test_auto_leave():
    st, rs = one([(0, 0), (1, 1)], last=10, committed=8, state=rdm.ST_LEADER)
    rs.applied[0] = 3
    (rec,), _ = rdm.ready(st, rs)
    for pci, want in ((2, rdm.ADV_OK), (3, rdm.ADV_OK | rdm.ADV_AUTO_LEAVE),
                      (8, rdm.ADV_OK | rdm.ADV_AUTO_LEAVE), (9, rdm.ADV_OK)):
        rs.applied[0] = 3
        assert rdm.advance(st, rs, [rec], auto_leave=[1], pending_conf_index=[pci]) == [want]
    rs.applied[0] = 3
    assert rdm.advance(st, rs, [rec], auto_leave=[0], pending_conf_index=[5]) == [rdm.ADV_OK]
    st.state[0], rs.applied[0] = 0, 3
    assert rdm.advance(st, rs, [rec], auto_leave=[1], pending_conf_index=[5]) == [rdm.ADV_OK]


# ---- the trace replay ----
@pytest.mark.parametrize("name", tc.MANDATORY)
def test_every_ready_block_from_the_records(blocks, name):
    r = rsim.replay(name, blocks)
    plain = tc.replay(name)
    assert r.compared == rsim.BLOCKS[name] == r.checked["readies"] == plain.checked["readies"]
    assert r.checked == plain.checked and dict(r.sent) == dict(plain.sent)


def leaves(name, **kw):
    with pytest.raises(tc.TraceMismatch) as e:
        rsim.replay(name, **kw)
    assert e.value.trace == name
    return e.value.line, str(e.value)


def test_control_without_the_note():
    """Without qe_ready_note a follower whose stable entries were truncated
    keeps its cursor past them (probe_and_replicate.txt, `stabilize 1 2`, line
    572: the entries 19.. rewritten under node 2), and a restored snapshot is
    never listed (snapshot_succeed_via_app_resp.txt, line 106)."""
    assert leaves("probe_and_replicate.txt", note=False)[0] == 572
    assert leaves("snapshot_succeed_via_app_resp.txt", note=False)[0] == 106


def test_control_stable_not_advanced():
    """An advance that leaves `stable` alone lists the same entries again."""
    line, what = leaves("campaign.txt", move_stable=False)
    assert line == 25 and "entries" in what
    assert leaves("confchange_v1_remove_leader.txt", move_stable=False)[0] == 73


def test_control_must_sync_from_commit():
    """MustSync from the whole HardState: a commit advance alone asks for a
    sync the reference does not (MustSync compares Term and Vote only)."""
    for name, at in (("campaign.txt", 25), ("snapshot_succeed_via_app_resp.txt", 106),
                     ("confchange_v1_remove_leader.txt", 73)):
        line, what = leaves(name, sync_from_commit=True)
        assert line == at and "must_sync" in what


# ---- the closed loop on the cluster simulation ----
def test_storage_rebuilt_from_the_records_alone():
    """tests/cluster_sim row c (one cluster, 275 rounds of a faulty network) with
    ready + advance every round: the stored log and HardState equal the
    resident ones at the end, the applied ranges have no gap, and the run saw
    truncated stable entries and snapshots."""
    from tests import cluster_sim as cs

    p = cs.ROWS["c"]
    s = rsim.ReadySim(p, rsim.ClusterReadyModel(p)).run()
    assert s.seen["truncations"] and s.seen["snapshots"] and s.seen["applied"]
    plain = cs.Sim(p, cs.ModelBackend(p)).run()
    assert s.counters()["cov"] == plain.counters()["cov"]  # the same schedule ran
    # without the note the truncated entries are never written again
    with pytest.raises(rsim.StorageMismatch):
        be = rsim.ClusterReadyModel(p)
        be.note = False
        rsim.ReadySim(p, be).run()
