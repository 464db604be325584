"""tests/outbox_model.py, the restatement of qe_outbox's rules, against the
safety-proven host rule it replaces (duty H7 of tests/cluster_sim.py, Sim.emit)
and on hand cases.  No GPU."""
import numpy as np
import pytest

from tests import cluster_sim as cs
from tests import outbox_model as om
from tests import outbox_sim as osim


# ---- (a) the model against Sim.emit, over the faulty-network runs ----
@pytest.fixture(scope="module")
def plain():
    return {}


def plain_counters(cache, name, p):
    if name not in cache:
        cache[name] = cs.Sim(p, cs.ModelBackend(p)).run().counters()
    return cache[name]


@pytest.mark.parametrize("name", sorted(cs.ROWS))
def test_model_matches_host_rule(plain, name):
    """Every MsgApp / MsgSnap / MsgHeartbeat the simulation's host layer builds
    equals the model's record for (sender, slot); every record is taken; the
    schedule is the plain run's."""
    p = cs.ROWS[name]
    sim = osim.OutboxSim(p, osim.ModelOutbox(p)).run()
    assert sim.counters() == plain_counters(plain, name, p)
    for k in ("app", "app_empty", "app_two_runs", "heartbeat", "snap"):
        assert sim.sent_cov[k] > 0, (k, dict(sim.sent_cov))


def test_reduced_row_a_shows_every_kind(plain):
    """The reduced row of tests/test_gpu_outbox_cluster.py on the models alone:
    a MsgSnap, a MsgApp of two or more runs, one cut at QE_MAX_MSG_RUNS, an
    empty one and a heartbeat all occur."""
    p = cs.ROWS["a"].but(**osim.ROW_A_SMALL)
    sim = osim.OutboxSim(p, osim.ModelOutbox(p)).run()
    assert sim.counters() == plain_counters(plain, "a_small", p)
    for k in osim.REQUIRED:
        assert sim.sent_cov[k] > 0, (k, dict(sim.sent_cov))


def test_rebuilt_messages_run_the_same_schedule(plain):
    """With the messages on the network rebuilt from the records the run is the
    plain run (what tests/test_gpu_outbox_cluster.py does with the device's)."""
    p = cs.ROWS["c"]
    sim = osim.OutboxSim(p, osim.ModelOutbox(p), rebuild=True).run()
    assert sim.counters() == plain_counters(plain, "c", p)


# ---- (c) the negative control ----
def test_swapped_replicate_rule_fails():
    """Next AFTER the call for a replicating peer (and before it for a probing
    one) is not the message's Index: row "a" notices."""
    p = cs.ROWS["a"]
    with pytest.raises(osim.OutboxMismatch):
        osim.OutboxSim(p, osim.ModelOutbox(p, replicate_before=False)).run()


# ---- (b) hand cases ----
RUNS = [(10, 2), (13, 3), (14, 5), (20, 6), (21, 9), (30, 11)]  # dummy 10, last_index 33
LAST = 33


def one_group(runs=RUNS, last=LAST, S=3, committed=12, **kw):
    """One group (stride 2: a pad column) with the run table `runs`."""
    R, st = max(len(runs), 1), 2
    rf, rt = np.zeros(R * st, np.uint64), np.zeros(R * st, np.uint64)
    for r, (f, t) in enumerate(runs):
        rf[r * st], rt[r * st] = f, t
    d = dict(num_groups=1, group_offset=1 << 33, num_slots=S, stride=st, log_runs=R,
             committed=[committed], last_index=[last], run_first=rf, run_term=rt,
             run_count=[len(runs)], snap_index=[11], first_index=[runs[0][0] + 1 if runs else 1])
    d.update(kw)
    return om.state(**d)


def app_to_slot0(index, msg_runs=4, max_entries=0, **kw):
    st = one_group(**kw)
    idx = np.zeros(st.num_slots * st.stride, np.uint64)
    idx[0] = index
    recs, stats = om.build(st, om.inputs(sent=[1], index=idx, term=[12], max_entries=max_entries),
                           msg_runs)
    assert len(recs) == 1
    return recs[0], stats


def test_index_at_the_dummy_entry():
    r, _ = app_to_slot0(10, msg_runs=2)
    assert (r["type"], r["index"], r["log_term"], r["commit"]) == (om.APP, 10, 2, 12)
    assert r["ents"] == [(2, 2), (1, 3)] and (r["group"], r["to"], r["term"]) == (1 << 33, 0, 12)


def test_index_at_last_index_is_an_empty_msgapp():
    r, stats = app_to_slot0(LAST)
    assert (r["type"], r["log_term"], r["ents"]) == (om.APP, 11, [])
    assert stats[om.STAT_APP] == 1 and stats[om.STAT_ENTRIES] == 0


@pytest.mark.parametrize("index", [9, LAST + 1])
def test_index_outside_the_log_is_bad(index):
    r, stats = app_to_slot0(index)
    assert r["type"] == om.BAD and r["index"] == index
    assert (r["log_term"], r["commit"], r["ctx"], r["ents"]) == (0, 0, 0, [])
    assert (r["group"], r["to"], r["term"]) == (1 << 33, 0, 12)
    assert stats[om.STAT_BAD] == stats[om.STAT_VIOLATIONS] == 1 and stats[om.STAT_APP] == 0


def test_empty_run_table_is_bad():
    r, _ = app_to_slot0(0, runs=[], last=0)
    assert r["type"] == om.BAD


@pytest.mark.parametrize("msg_runs,want", [
    (0, []), (1, [(1, 2)]), (4, [(1, 2), (1, 3), (6, 5), (1, 6)])])
def test_six_runs_cut_to_msg_runs(msg_runs, want):
    """Index 11 in a log of six runs: the message ends where its last listed
    run ends."""
    r, stats = app_to_slot0(11, msg_runs=msg_runs)
    assert r["ents"] == want and r["log_term"] == 2
    assert stats[om.STAT_ENTRIES] == sum(n for n, _ in want)


def test_max_entries_inside_a_run_and_on_a_boundary():
    r, _ = app_to_slot0(13, max_entries=3)      # (13, 16]: inside the run of term 5
    assert r["ents"] == [(3, 5)]
    r, _ = app_to_slot0(13, max_entries=6)      # (13, 19]: exactly the run of term 5
    assert r["ents"] == [(6, 5)]
    r, _ = app_to_slot0(13, max_entries=7)      # one entry of the next run
    assert r["ents"] == [(6, 5), (1, 6)]
    r, _ = app_to_slot0(LAST - 1, max_entries=7)  # the log ends first
    assert r["ents"] == [(1, 11)]


def test_snap_wins_over_sent_and_sent_over_heartbeat():
    st = one_group()
    n = st.num_slots * st.stride
    idx, hc = np.full(n, 12, np.uint64), np.full(n, 7, np.uint64)
    recs, stats = om.build(st, om.inputs(sent=[0b011], snap=[0b001], hb_sent=[0b111], index=idx,
                                         hb_commit=hc, hb_ctx=[5], term=[12]), 4)
    assert [(r["to"], r["type"]) for r in recs] == [(0, om.SNAP), (1, om.APP), (2, om.HEARTBEAT)]
    assert (recs[0]["index"], recs[0]["log_term"], recs[0]["commit"], recs[0]["ctx"]) == (11, 2, 0, 0)
    assert (recs[2]["index"], recs[2]["commit"], recs[2]["ctx"]) == (0, 7, 5)
    assert stats[om.STAT_GROUPS] == stats[om.STAT_SNAP] == stats[om.STAT_HEARTBEAT] == 1


def test_snap_term_given_and_not_given():
    st = one_group()
    r = om.build(st, om.inputs(snap=[1], term=[12], snap_term=[77]), 4)[0][0]
    assert (r["index"], r["log_term"]) == (11, 77)
    r = om.build(st, om.inputs(snap=[1], term=[12]), 4)[0][0]
    assert (r["index"], r["log_term"]) == (11, 2)
    r = om.build(one_group(snap_index=[5]), om.inputs(snap=[1], term=[12]), 4)[0][0]
    assert (r["index"], r["log_term"]) == (5, 0)        # below the log: term() is 0
    r = om.build(one_group(snap_index=None), om.inputs(snap=[1], term=[12]), 4)[0][0]
    assert r["index"] == 10                             # first_index - 1


def test_mask_bits_at_and_above_num_slots_are_ignored():
    st = one_group(S=3)
    idx = np.full(st.num_slots * st.stride, 12, np.uint64)
    recs, stats = om.build(st, om.inputs(sent=[0b11111100], index=idx, term=[12]), 4)
    assert [r["to"] for r in recs] == [2]
    recs, stats = om.build(st, om.inputs(sent=[0b11111000], index=idx, term=[12]), 4)
    assert recs == [] and stats[om.STAT_GROUPS] == 0


def test_next_rule_by_peer_state():
    st = one_group(S=2)
    n = st.num_slots * st.stride
    st.next, st.peer = np.full(n, 20, np.uint64), np.zeros(n, np.uint32)
    st.peer[st.stride] = 1 | 8 | (3 << 16)  # slot 1 replicates (with flag and ring bits set)
    before = np.full(n, 15, np.uint64)
    recs, _ = om.build(st, om.inputs(sent=[0b11], next_before=before, term=[12]), 4)
    assert [r["index"] for r in recs] == [19, 14]


def test_order_and_capacity():
    """Tile, then slot, then group; a list cut at capacity keeps the count."""
    G, S, st = 70, 2, 73
    sent = np.zeros(G, np.uint8)
    sent[[0, 5, 63, 64, 69]] = [3, 2, 1, 3, 1]
    rf = np.zeros(st, np.uint64)
    s = om.state(num_groups=G, num_slots=S, stride=st, log_runs=1, committed=np.zeros(G, np.uint64),
                 last_index=np.full(G, 9, np.uint64), run_first=rf, run_term=rf + 1,
                 run_count=np.ones(G, np.uint8))
    recs, stats = om.build(s, om.inputs(sent=sent, index=np.full(S * st, 4, np.uint64),
                                        term=np.ones(G, np.uint64)), 1)
    assert [(r["group"], r["to"]) for r in recs] == [(0, 0), (63, 0), (0, 1), (5, 1), (64, 0),
                                                     (69, 0), (64, 1)]
    assert all(r["ents"] == [(5, 1)] for r in recs) and stats[om.STAT_GROUPS] == 5
    for cap in (0, len(recs) - 1, len(recs)):
        count, kept = om.truncate(recs, cap)
        assert count == 7 and kept == recs[:cap]
