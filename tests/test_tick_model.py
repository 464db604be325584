"""tests/tick_model.py (the CPU restatement of raft.tick() that qe_tick is
checked against) pinned to the reference's own tests, transcribed as hand
cases, and qe_tick's argument errors (no GPU: validation precedes any launch)."""
import ctypes as C

import numpy as np

from etcd_amd import _lib
from tests import tick_model as tm


def one(S, state, et=10, ht=1, cq=False, voters=None, self_slot=0, tracked=None, seed=1):
    m = tm.Model(1, S, et, ht, cq, seed=seed)
    m.state[:] = state
    m.self_slot = np.array([self_slot], np.uint8)
    m.inc = np.array([(1 << S) - 1 if voters is None else voters], np.int64)
    m.tracked = None if tracked is None else np.array([tracked], np.int64)
    m.lead_transferee = np.array([tm.NONE], np.uint8)
    return m


def test_leader_transfer_timeout():
    """TestLeaderTransferTimeout (raft_test.go:3610): the transferee survives
    heartbeatTimeout ticks and is gone after electionTimeout."""
    m = one(3, tm.LEADER)
    m.lead_transferee[0] = 2
    for _ in range(m.ht):
        o = m.tick()
    assert m.lead_transferee[0] == 2 and not o.action[0] & tm.TRANSFER_ABORTED
    for _ in range(m.et - m.ht):
        o = m.tick()
    assert m.lead_transferee[0] == tm.NONE and m.state[0] == tm.LEADER
    assert o.action[0] & tm.TRANSFER_ABORTED and not o.action[0] & tm.STEPDOWN


def test_add_node_check_quorum():
    """TestAddNodeCheckQuorum (:3221): node 2 is added (RecentActive, as a new
    Progress is) one tick before the check; the check passes, and fails
    electionTimeout ticks later."""
    m = one(2, tm.LEADER, cq=True, voters=1, tracked=1)
    for _ in range(m.et - 1):
        o = m.tick()
        assert o.action[0] == tm.BEAT
    m.inc[0] = m.tracked[0] = 3
    m.peer[1] = tm.RECENT_ACTIVE
    o = m.tick()
    assert m.state[0] == tm.LEADER and o.quorum_active[0] == 1
    assert o.action[0] == tm.CHECKED_QUORUM | tm.BEAT
    assert m.peer[0] & tm.RECENT_ACTIVE and not m.peer[1] & tm.RECENT_ACTIVE
    for i in range(m.et):
        assert m.state[0] == tm.LEADER
        o = m.tick()
    assert m.state[0] == tm.FOLLOWER and o.quorum_active[0] == 0
    assert o.action[0] == tm.CHECKED_QUORUM | tm.STEPDOWN  # no beat on the stepdown tick
    assert m.ee[0] == 0 and m.he[0] == 0 and m.et <= m.rt[0] < 2 * m.et


def test_learner_election_timeout():
    """TestLearnerElectionTimeout (:324): a learner never hups."""
    m = one(2, tm.FOLLOWER, voters=1, self_slot=1)  # slot 1 is tracked, not a voter
    for _ in range(3 * m.et):
        assert m.tick().action[0] == 0
    assert m.ee[0] == 3 * m.et


def test_non_promotable_voter_with_check_quorum():
    """TestNonPromotableVoterWithCheckQuorum (:1942): b removed itself from its
    own config (no Progress of its own): electionTimeout ticks, no campaign."""
    m = one(2, tm.FOLLOWER, cq=True, voters=1, self_slot=1, tracked=1)
    m.rt[0] = m.et + 1
    assert not m.promotable()[0]
    for _ in range(m.et + 5):
        assert m.tick().action[0] == 0
    assert m.state[0] == tm.FOLLOWER


def test_leader_bcast_beat():
    """TestLeaderBcastBeat (raft_paper_test.go:109): one beat per
    heartbeatTimeout ticks, to every peer but the leader."""
    ht = 3
    m = one(3, tm.LEADER, et=10, ht=ht, self_slot=0)
    m.match[:] = [9, 5, 20]
    m.committed[0] = 7
    beats = 0
    for i in range(1, 3 * ht + 1):
        o = m.tick(out=tm.TickOut(m, sentinel=0xEE))
        if i % ht == 0:
            beats += 1
            assert o.action[0] == tm.BEAT and o.hb_sent[0] == 0b110
            assert list(o.hb_commit) == [0xEE, 5, 7]  # min(Match, committed); not to self
        else:
            assert o.action[0] == 0 and o.hb_sent[0] == 0 and list(o.hb_commit) == [0xEE] * 3
    assert beats == 3


def test_follower_and_candidate_start_election():
    """TestFollowerStartElection / TestCandidateStartNewElection
    (raft_paper_test.go:134-139): a HUP after 2 * electionTimeout ticks at
    the latest, never before electionTimeout."""
    for state in (tm.FOLLOWER, tm.CANDIDATE, tm.PRE_CANDIDATE):
        for seed in range(20):
            m = one(3, state, seed=seed)
            m.reset(np.array([True]))
            first = None
            for i in range(1, 2 * m.et + 1):
                if m.tick().action[0] & tm.HUP:
                    first = i
                    break
            assert first is not None and m.et <= first <= 2 * m.et - 1 and m.ee[0] == 0


def test_past_election_timeout():
    """TestPastElectionTimeout (raft_test.go:1176) over 10,000 groups' draws
    at electionTimeout 10 (fixed seed: deterministic)."""
    G, et = 10000, 10
    m = tm.Model(G, 1, et, 1, False, seed=0x5EED)
    m.reset(np.ones(G, bool))
    assert set(np.unique(m.rt)) == set(range(et, 2 * et))
    for elapse, want, rnd in ((5, 0, False), (10, .1, True), (13, .4, True), (15, .6, True),
                              (18, .9, True), (20, 1, False)):
        m.ee[:] = elapse
        got = m.past_election_timeout().sum() / G
        if rnd:
            got = np.floor(got * 10 + 0.5) / 10.0
        assert got == want, (elapse, got)
    # the draw is a function of (seed, global group id, tick number) alone
    m2 = tm.Model(100, 1, et, 1, False, seed=0x5EED, goff=500)
    m2.reset(np.ones(100, bool))
    assert np.array_equal(m2.rt, m.rt[500:600])
    m2.tick_no = 1
    m2.reset(np.ones(100, bool))
    assert not np.array_equal(m2.rt, m.rt[500:600])


def test_events_and_saturation():
    """HEARD clears electionElapsed, RESET wins over it and draws again;
    ticks = 0 applies events alone; the device form saturates at 65535."""
    m = tm.Model(4, 1, 10, 1, False, seed=3)
    m.ee[:] = [5, 5, 5, 65534]
    m.he[:] = 2
    o = m.tick(events=np.array([0, 1, 3, 0], np.uint8), ticks=0)
    assert list(m.ee) == [5, 0, 0, 65534] and list(m.he) == [2, 2, 0, 2]
    assert not o.action.any() and m.tick_no == 0
    m.tick()
    m.tick()
    assert m.ee[3] == 65536 and m.timer()[3] & 0xFFFF == 0xFFFF  # nobody promotable here


V = C.c_void_p(64)


def tick_rc(p=None, t=None, o=None, **kw):
    pk = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4)
    tk = dict(state=V, timer=V, randomized_timeout=V, election_timeout=10, heartbeat_timeout=1,
              ticks=1)
    ok = dict(action=V)
    pk.update(p or {})
    tk.update(t or {})
    ok.update(o or {})
    return _lib.lib().qe_tick(C.byref(_lib.QeProgress(**pk)), C.byref(_lib.QeTimers(**tk)),
                              C.byref(_lib.QeTickOut(**ok)), None, None)


def test_tick_argument_errors_without_gpu():
    L, E = _lib.lib(), _lib.QE_EINVAL
    p, t, o = _lib.QeProgress(num_groups=4, num_slots=3, stride=4), _lib.QeTimers(), _lib.QeTickOut()
    assert L.qe_tick(None, C.byref(t), C.byref(o), None, None) == E
    assert L.qe_tick(C.byref(p), None, C.byref(o), None, None) == E
    assert L.qe_tick(C.byref(p), C.byref(t), None, None, None) == E
    for k in ("state", "timer", "randomized_timeout"):
        assert tick_rc(t={k: None}) == E, k
    assert tick_rc(o={"action": None}) == E
    for k, bad in (("election_timeout", 0), ("election_timeout", 32769),
                   ("heartbeat_timeout", 0), ("heartbeat_timeout", 65536)):
        assert tick_rc(t={k: bad}) == E, (k, bad)
    assert tick_rc(t={"flags": 2}) == E and tick_rc(t={"flags": 3}) == E
    assert tick_rc(t={"ticks": 2}) == E
    assert tick_rc(p={"out_mask": V}) == E  # out_mask without inc_mask
    assert tick_rc(t={"flags": _lib.QE_TICK_CHECK_QUORUM}) == E  # CheckQuorum, no peer words
    assert tick_rc(o={"hb_commit": V}) == E  # no match / committed
    assert tick_rc(p={"match": V}, o={"hb_commit": V}) == E
    assert tick_rc(p={"match": V, "committed": V, "stride": 3}, o={"hb_commit": V}) == E
    assert tick_rc(p={"read_acks": V}) == E  # a queue comes whole
    assert tick_rc(p={"read_acks": V, "read_head": V}) == E
    assert tick_rc(p={"num_slots": 0}) == E and tick_rc(p={"num_slots": 17}) == E
    # an empty batch is a no-op, whatever else is missing
    assert tick_rc(p={"num_groups": 0, "stride": 0}, t={"state": None}) == _lib.QE_OK
    assert _lib.QE_ABI_VERSION == 8  # additive: the ABI version stays
