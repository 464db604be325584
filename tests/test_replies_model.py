"""tests/replies_model.py, the restatement of qe_replies' rules, against the
safety-proven host rules it replaces (duty H8 and the vote half of H4 of
tests/cluster_sim.py: Sim.do_follow / do_snap / do_vote) and on hand cases.
No GPU."""
import numpy as np
import pytest

from tests import cluster_sim as cs
from tests import inbox_sim
from tests import replies_model as rm
from tests import replies_sim as rsim


# ---- (a) the model against the host rules, over the faulty-network runs ----
@pytest.fixture(scope="module")
def plain():
    return {}


def plain_run(cache, name, p):
    if name not in cache:
        cache[name] = cs.Sim(p, cs.ModelBackend(p)).run()
    return cache[name]


SMALL = {"c": cs.ROWS["c"], "b_small": cs.ROWS["b"].but(**inbox_sim.ROW_B_SMALL)}


@pytest.mark.parametrize("name", sorted(cs.ROWS))
def test_model_matches_host_rule(plain, name):
    """Every response and vote message the simulation's host layer builds equals
    the model's record for (sender, slot, type); every record is taken; the
    schedule is the plain run's."""
    p = cs.ROWS[name]
    be = rsim.ModelReplies(p)
    sim = rsim.RepliesSim(p, be).run()
    assert sim.counters() == plain_run(plain, name, p).counters()
    assert be.listed == sum(sim.sent_cov.values()) > 0


# The occurrences in Sim.cov of the stock simulation on the two rows of
# tests/test_gpu_replies_cluster.py.
COV = {
    "c": dict(FR_APP_ACCEPT=186, FR_APP_REJECT=34, FR_APP_STALE=11, FR_HEARTBEAT_RESP=142,
              FR_LOWER_TERM_RESP=20, SR_STALE=1, SR_RESTORED=4, VR_GRANT=12, VR_REJECT=56,
              VR_CAMPAIGN_VOTE=82, VR_CAMPAIGN_PREVOTE=0),
    "b_small": dict(FR_APP_ACCEPT=631, FR_APP_REJECT=51, FR_APP_STALE=33, FR_HEARTBEAT_RESP=509,
                    FR_LOWER_TERM_RESP=3, SR_STALE=0, SR_RESTORED=2, VR_GRANT=113, VR_REJECT=72,
                    VR_CAMPAIGN_VOTE=20, VR_CAMPAIGN_PREVOTE=68),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_gpu_loop_rows_show_every_kind(plain, name):
    """The two rows of the GPU loop test on the models alone: the stock run
    shows the result codes counted above, and the records cover every kind the
    row must show."""
    p = SMALL[name]
    ref = plain_run(plain, name, p)
    assert {k: ref.cov.get(k, 0) for k in COV[name]} == COV[name]
    sim = rsim.RepliesSim(p, rsim.ModelReplies(p)).run()
    assert sim.counters() == ref.counters()
    for k in rsim.REQUIRED_BY_ROW[name]:
        assert sim.sent_cov[k] > 0, (k, dict(sim.sent_cov))
    # one response per answering result, the duplicates of the network apart
    c = sim.sent_cov
    assert c["app_accept"] == COV[name]["FR_APP_ACCEPT"]
    assert c["app_reject"] == COV[name]["FR_APP_REJECT"]
    assert c["heartbeat_resp"] == COV[name]["FR_HEARTBEAT_RESP"]
    assert c["snap_resp"] == COV[name]["SR_STALE"] + COV[name]["SR_RESTORED"]
    assert c["vote_grant"] + c["vote_reject"] + c["prevote_resp"] == \
        COV[name]["VR_GRANT"] + COV[name]["VR_REJECT"]


# ---- (c) rebuilt messages ----
def test_rebuilt_messages_run_the_same_schedule(plain):
    """With the messages on the network rebuilt from the records the run is the
    plain run (what tests/test_gpu_replies_cluster.py does with the device's)."""
    p = cs.ROWS["c"]
    sim = rsim.RepliesSim(p, rsim.ModelReplies(p), rebuild=True).run()
    assert sim.counters() == plain_run(plain, "c", p).counters()


# ---- (d) the negative control ----
def test_dropped_reject_hint_fails():
    """A reject record without its RejectHint is not the message the host rule
    builds: row "c" notices."""
    p = cs.ROWS["c"]
    with pytest.raises(rsim.RepliesMismatch):
        rsim.RepliesSim(p, rsim.ModelReplies(p, drop_hint=True)).run()


# ---- (e) hand cases ----
GOFF = 1 << 33


def st_of(G=1, S=3, last=None):
    return rm.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=G + 2,
                    last_index=last if last is not None else [40 + g for g in range(G)])


def follow_inp(result, frm=1, **kw):
    d = dict(term=[7], f_result=[result], f_from=[frm], f_resp_index=[21], f_reject_hint=[19],
             f_resp_log_term=[5])
    d.update(kw)
    return rm.inputs(**d)


def fields(r, *names):
    return tuple(r[k] for k in names)


@pytest.mark.parametrize("result,want", [
    (rm.FR_LOWER_TERM_RESP, (rm.APP_RESP, 0, 0, 0, 0)),
    (rm.FR_HEARTBEAT_RESP, (rm.HEARTBEAT_RESP, 0, 0, 0, 0)),
    (rm.FR_APP_ACCEPT, (rm.APP_RESP, 21, 0, 0, 0)),
    (rm.FR_APP_STALE, (rm.APP_RESP, 21, 0, 0, 0)),
    (rm.FR_APP_REJECT, (rm.APP_RESP_REJECT, 21, 19, 5, 0)),
])
def test_follower_results_that_answer(result, want):
    recs, stats = rm.build(st_of(), follow_inp(result))
    assert len(recs) == 1
    r = recs[0]
    assert fields(r, "type", "index", "hint", "log_term", "flags") == want
    assert fields(r, "group", "to", "term", "ctx") == (GOFF, 1, 7, 0)
    which = rm.STAT_HEARTBEAT_RESP if result == rm.FR_HEARTBEAT_RESP else rm.STAT_APP_RESP
    assert stats[which] == stats[rm.STAT_GROUPS] == 1 and stats[rm.STAT_BAD] == 0


@pytest.mark.parametrize("result", [0, 1, 7, 15, 16, 17, 18, 19, 20, 255])
def test_follower_results_that_yield_nothing(result):
    """NONE, IGNORED, unknown codes and every refused result (>= 16)."""
    recs, stats = rm.build(st_of(), follow_inp(result))
    assert recs == [] and stats[rm.STAT_GROUPS] == 0


def test_heartbeat_ctx_null_and_given():
    assert rm.build(st_of(), follow_inp(rm.FR_HEARTBEAT_RESP))[0][0]["ctx"] == 0
    r = rm.build(st_of(), follow_inp(rm.FR_HEARTBEAT_RESP, f_ctx=[0xFEDCBA98]))[0][0]
    assert r["ctx"] == 0xFEDCBA98
    # the context belongs to the heartbeat response alone
    assert rm.build(st_of(), follow_inp(rm.FR_APP_ACCEPT, f_ctx=[9]))[0][0]["ctx"] == 0


@pytest.mark.parametrize("result,n", [(0, 0), (1, 0), (rm.SR_STALE, 1), (rm.SR_NOT_MEMBER, 1),
                                      (rm.SR_FAST_FORWARD, 1), (rm.SR_RESTORED, 1), (6, 0),
                                      (16, 0), (17, 0), (18, 0)])
def test_snapshot_results(result, n):
    recs, stats = rm.build(st_of(), rm.inputs(term=[7], s_result=[result], s_from=[2],
                                              s_resp_index=[33]))
    assert len(recs) == n == stats[rm.STAT_APP_RESP]
    if n:
        assert fields(recs[0], "type", "to", "term", "index", "hint", "log_term", "ctx",
                      "flags") == (rm.APP_RESP, 2, 7, 33, 0, 0, 0, 0)


def vote_inp(result, vtype=rm.VMSG_VOTE, frm=2, req_to=0b101, **kw):
    d = dict(term=[99], v_result=[result], v_type=[vtype], v_from=[frm], v_resp_term=[8],
             v_req_log_term=[6], v_req_to=[req_to])
    d.update(kw)
    return rm.inputs(**d)


@pytest.mark.parametrize("result,vtype,want", [
    (rm.VR_GRANT, rm.VMSG_VOTE, (rm.VOTE_RESP, 0)),
    (rm.VR_REJECT, rm.VMSG_VOTE, (rm.VOTE_RESP, rm.VMF_REJECT)),
    (rm.VR_GRANT, rm.VMSG_PREVOTE, (rm.PREVOTE_RESP, 0)),
    (rm.VR_REJECT, rm.VMSG_PREVOTE, (rm.PREVOTE_RESP, rm.VMF_REJECT)),
])
def test_vote_responses(result, vtype, want):
    recs, stats = rm.build(st_of(), vote_inp(result, vtype))
    assert len(recs) == 1 == stats[rm.STAT_VOTE_RESP]
    assert fields(recs[0], "type", "flags") == want
    # the term is resp_term, not the term row
    assert fields(recs[0], "to", "term", "index", "log_term", "hint", "ctx") == (2, 8, 0, 0, 0, 0)


@pytest.mark.parametrize("result", [0, 1, 2, 5, 6, 7, 10, 11, 16, 200])
def test_vote_results_that_yield_nothing(result):
    """NONE, IGNORED, IN_LEASE, STEPPED_DOWN, PENDING, LOST, WON, refused."""
    recs, stats = rm.build(st_of(), vote_inp(result))
    assert recs == [] and stats[rm.STAT_GROUPS] == 0


@pytest.mark.parametrize("vtype", [0, 3, 4, 5, 6, 77])
def test_grant_for_a_message_that_is_no_request_is_bad(vtype):
    for result in (rm.VR_GRANT, rm.VR_REJECT):
        recs, stats = rm.build(st_of(), vote_inp(result, vtype))
        assert fields(recs[0], "type", "to", "term", "flags", "index") == (rm.BAD, 2, 8, 0, 0)
        assert stats[rm.STAT_BAD] == stats[rm.STAT_VIOLATIONS] == 1
        assert stats[rm.STAT_VOTE_RESP] == 0 and stats[rm.STAT_GROUPS] == 1


@pytest.mark.parametrize("frm", [3, 4, 0xFF])
def test_to_that_is_no_slot_is_bad(frm):
    """S = 3: the record keeps group, to and term; every other field is 0."""
    for inp in (follow_inp(rm.FR_APP_REJECT, frm), follow_inp(rm.FR_HEARTBEAT_RESP, frm, f_ctx=[5]),
                rm.inputs(term=[7], s_result=[rm.SR_RESTORED], s_from=[frm], s_resp_index=[33]),
                vote_inp(rm.VR_REJECT, frm=frm)):
        recs, stats = rm.build(st_of(), inp)
        assert len(recs) == 1
        r = recs[0]
        assert fields(r, "type", "group", "to") == (rm.BAD, GOFF, frm)
        assert r["term"] == (8 if inp.v_result is not None else 7)
        assert fields(r, "index", "hint", "log_term", "ctx", "flags") == (0, 0, 0, 0, 0)
        assert stats[rm.STAT_BAD] == stats[rm.STAT_VIOLATIONS] == 1
        assert stats[rm.STAT_APP_RESP] == stats[rm.STAT_HEARTBEAT_RESP] == 0


@pytest.mark.parametrize("result,vtype,ty,flags", [
    (rm.VR_CAMPAIGN_VOTE, 5, rm.VOTE, 0),
    (rm.VR_CAMPAIGN_VOTE, rm.VMSG_TIMEOUT_NOW, rm.VOTE, rm.VMF_FORCE),
    (rm.VR_CAMPAIGN_PREVOTE, 5, rm.PREVOTE, 0),
    (rm.VR_CAMPAIGN_PREVOTE, rm.VMSG_TIMEOUT_NOW, rm.PREVOTE, 0),  # FORCE is an election's alone
    (rm.VR_CAMPAIGN_VOTE, 4, rm.VOTE, 0),  # the pre-vote won (a QE_VMSG_PREVOTE_RESP)
])
def test_campaign_requests_and_force(result, vtype, ty, flags):
    recs, stats = rm.build(st_of(last=[41]), vote_inp(result, vtype, frm=0xFF))
    assert [r["to"] for r in recs] == [0, 2]  # v_from is not read: no BAD
    for r in recs:
        assert fields(r, "type", "term", "index", "log_term", "flags", "hint", "ctx") == \
            (ty, 8, 41, 6, flags, 0, 0)
    assert stats[rm.STAT_VOTE_REQ] == 2 and stats[rm.STAT_GROUPS] == 1


def test_mask_bits_at_and_above_num_slots_are_ignored():
    recs, _ = rm.build(st_of(S=3), vote_inp(rm.VR_CAMPAIGN_VOTE, 5, req_to=0b11111100))
    assert [r["to"] for r in recs] == [2]
    recs, stats = rm.build(st_of(S=3), vote_inp(rm.VR_CAMPAIGN_VOTE, 5, req_to=0b11111000))
    assert recs == [] and stats[rm.STAT_GROUPS] == 0
    recs, _ = rm.build(st_of(S=3), rm.inputs(term=[7], timeout_now=[0b11111010]))
    assert [(r["to"], r["type"], r["term"]) for r in recs] == [(1, rm.TIMEOUT_NOW, 7)]
    recs, stats = rm.build(st_of(S=3), rm.inputs(term=[7], timeout_now=[0b11111000]))
    assert recs == [] and stats[rm.STAT_GROUPS] == 0


def test_absent_families_yield_nothing():
    recs, stats = rm.build(st_of(), rm.inputs(term=[7]))
    assert recs == [] and not any(stats.values())


def test_a_group_with_all_five_kinds_at_once():
    inp = rm.inputs(term=[7], f_result=[rm.FR_APP_ACCEPT], f_from=[1], f_resp_index=[21],
                    f_reject_hint=[0], f_resp_log_term=[0], s_result=[rm.SR_STALE], s_from=[0],
                    s_resp_index=[33], v_result=[rm.VR_CAMPAIGN_VOTE], v_type=[5], v_from=[0],
                    v_resp_term=[8], v_req_log_term=[6], v_req_to=[0b110], timeout_now=[0b001])
    recs, stats = rm.build(st_of(last=[41]), inp)
    assert [(r["type"], r["to"]) for r in recs] == [
        (rm.APP_RESP, 1), (rm.APP_RESP, 0), (rm.VOTE, 1), (rm.VOTE, 2), (rm.TIMEOUT_NOW, 0)]
    assert stats[rm.STAT_GROUPS] == 1 and stats[rm.STAT_APP_RESP] == 2
    assert stats[rm.STAT_VOTE_REQ] == 2 and stats[rm.STAT_TIMEOUT_NOW] == 1
    # a response and a campaign exclude each other: one result per group
    inp.v_result = [rm.VR_GRANT]
    inp.v_type = [rm.VMSG_VOTE]
    recs, _ = rm.build(st_of(last=[41]), inp)
    assert [(r["type"], r["to"]) for r in recs] == [
        (rm.APP_RESP, 1), (rm.APP_RESP, 0), (rm.VOTE_RESP, 0), (rm.TIMEOUT_NOW, 0)]


def test_order_and_capacity():
    """Tile, then kind, then (for the mask kinds) slot, then group; a list cut
    at capacity keeps the count."""
    G, S = 70, 2
    z8, z64 = np.zeros(G, np.uint8), np.zeros(G, np.uint64)
    fr, sr, vr, tn, req = z8.copy(), z8.copy(), z8.copy(), z8.copy(), z8.copy()
    fr[[0, 63, 64]] = rm.FR_APP_ACCEPT
    sr[[5, 69]] = rm.SR_RESTORED
    vr[[0, 5, 64]] = [rm.VR_CAMPAIGN_VOTE, rm.VR_GRANT, rm.VR_CAMPAIGN_VOTE]
    req[[0, 64]] = [3, 2]
    tn[[5, 63, 69]] = [3, 1, 2]
    inp = rm.inputs(term=z64 + 4, f_result=fr, f_from=z8 + 1, f_resp_index=z64, f_reject_hint=z64,
                    f_resp_log_term=z64, s_result=sr, s_from=z8, s_resp_index=z64, v_result=vr,
                    v_type=z8 + 1, v_from=z8, v_resp_term=z64 + 5, v_req_log_term=z64,
                    v_req_to=req, timeout_now=tn)
    recs, stats = rm.build(rm.state(num_groups=G, num_slots=S, stride=73, last_index=z64), inp)
    A, VQ, VR, T = rm.APP_RESP, rm.VOTE, rm.VOTE_RESP, rm.TIMEOUT_NOW
    assert [(r["group"], r["type"], r["to"]) for r in recs] == [
        (0, A, 1), (63, A, 1), (5, A, 0), (5, VR, 0), (0, VQ, 0), (0, VQ, 1), (5, T, 0),
        (63, T, 0), (5, T, 1),
        (64, A, 1), (69, A, 0), (64, VQ, 1), (69, T, 1)]
    assert stats[rm.STAT_GROUPS] == 5
    for cap in (0, len(recs) - 1, len(recs)):
        count, kept = rm.truncate(recs, cap)
        assert count == 13 and kept == recs[:cap]
