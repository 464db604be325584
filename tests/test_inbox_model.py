"""tests/inbox_model.py, the sequential restatement of qe_inbox's rules,
against the host rule it replaces (duties H4, H6 and H1's HUP of
tests/cluster_sim.py, Sim.deliver) and on hand cases.  With qe_inbox those
duties are optional for a host.  No GPU."""
import numpy as np
import pytest

from tests import cluster_sim as cs
from tests import inbox_model as im
from tests import inbox_sim as isim

ROWS = dict(cs.ROWS, b_small=cs.ROWS["b"].but(**isim.ROW_B_SMALL))


@pytest.fixture(scope="module")
def runs():
    """name -> (the stock run, the inbox run), each computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            p = ROWS[name]
            cache[name] = (isim.StockSim(p, cs.ModelBackend(p)).run(),
                           isim.InboxSim(p, cs.ModelBackend(p)).run())
        return cache[name]
    return get


# ---- (a) the model against Sim.deliver, over the faulty-network runs ----
@pytest.mark.parametrize("name", sorted(ROWS))
def test_model_matches_host_rule(runs, name):
    """Every call of the run gets the rows the stock Sim.deliver builds; the
    schedule, the discards and the leaders are the stock run's; every list
    record got exactly one disposition (InboxSim.deliver asserts it)."""
    stock, sim = runs(name)
    assert len(sim.calls_seen) == len(stock.calls_seen)
    for k, (a, b) in enumerate(zip(sim.calls_seen, stock.calls_seen)):
        assert a == b, (k, a, b)
    assert sim.counters() == stock.counters()
    assert sim.discards == stock.discards
    assert sim.inv.leaders == stock.inv.leaders
    d = sim.dispositions
    assert d["DROP_LOWER_TERM"] == stock.discards["resp_lower_term"]
    assert d["DROP_NOT_LEADER"] == (stock.discards["resp_not_leader"] +
                                    stock.discards["snap_status_not_leader"])
    assert d["STEPDOWN"] == stock.cov["resp_higher_term"]
    assert d["BAD"] == 0 and d["ROUTED"] > 0 and d["DEFERRED"] > 0


def test_gpu_rows_show_every_kind(runs):
    """Row "c" and the reduced row "b" of tests/test_gpu_inbox_cluster.py
    together: joined responses, waves of three or more, a wave closed by a
    second response of one slot and one closed by another class, a higher-term
    conversion, a lower-term drop and a not-leader drop all occur."""
    for name, keys in isim.REQUIRED_BY_ROW.items():
        kinds = runs(name)[1].kinds
        for k in keys:
            assert kinds[k] > 0, (name, k, dict(kinds))


# ---- (c) the negative control ----
def test_same_slot_response_joining_the_wave_is_caught(runs):
    """A variant that lets a second response of one slot join the wave (it
    overwrites the first in its cell) does not run the stock schedule."""
    p = ROWS["b_small"]
    stock = runs("b_small")[0]
    try:
        sim = isim.InboxSim(p, cs.ModelBackend(p), same_from_joins=True).run()
    except AssertionError:
        return
    assert sim.calls_seen != stock.calls_seen


# ---- (b) hand cases: one group unless said otherwise, S = 3 ----
GOFF = 1 << 33


def st(term=5, state=im.ST_LEADER, G=1, S=3):
    return im.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=G + 3,
                    term=[term] * G, state=[state] * G)


def R(frm, term=5, type=im.APP_RESP, g=0, **kw):
    return im.rec(GOFF + g, frm, type, term, **kw)


def test_routed_follower_snapshot_vote():
    s = st(G=3)
    recs = [im.rec(GOFF + 0, 1, im.APP, 7, 10, 6, 9, ents=[(2, 6), (1, 7)]),
            im.rec(GOFF + 1, 2, im.SNAP, 7, 20, 6),
            im.rec(GOFF + 2, 0, im.PREVOTE, 8, 30, 6, flags=1),
            im.rec(GOFF + 0, 1, im.HEARTBEAT, 7, commit=9)]
    o = im.route(s, recs, msg_runs=4)
    assert o.disposition == [im.ROUTED, im.ROUTED, im.ROUTED, im.DEFERRED] and o.deferred == [3]
    assert o.f == {0: dict(type=im.LMSG_APP, frm=1, term=7, index=10, log_term=6, commit=9,
                           ents=[(2, 6), (1, 7), (0, 0), (0, 0)], src=0)}
    assert o.s == {1: dict(type=im.SMSG_SNAP, frm=2, term=7, snap_index=20, snap_term=6, src=1)}
    assert o.v == {2: dict(type=2, frm=0, term=8, index=30, log_term=6, flags=1, src=2)}
    assert o.r == {} and o.stats[im.STAT_GROUPS] == 3 and o.stats[im.STAT_ROUTED] == 3
    # the deferred heartbeat is routed by the next pass: no entry rows for it
    o = im.route(s, [recs[3]])
    assert o.f[0]["type"] == im.LMSG_HEARTBEAT and o.f[0]["ents"] is None


def test_response_wave_joins_until_a_slot_repeats():
    recs = [R(0, index=11), R(2, type=im.HEARTBEAT_RESP, ctx=7), R(1, type=im.APP_RESP_REJECT,
                                                                   index=12, hint=9, log_term=4),
            R(2, index=13), R(1, index=14)]
    o = im.route(st(), recs)
    assert o.disposition == [im.ROUTED] * 3 + [im.DEFERRED] * 2 and o.deferred == [3, 4]
    assert o.r == {(0, 0): dict(type=1, index=11, hint=0, log_term=0, ctx=0, src=0),
                   (2, 0): dict(type=3, index=0, hint=0, log_term=0, ctx=7, src=1),
                   (1, 0): dict(type=2, index=12, hint=9, log_term=4, ctx=0, src=2)}
    assert o.stats[im.STAT_GROUPS] == 1 and o.stats[im.STAT_DEFERRED] == 2


def test_another_class_closes_a_response_wave():
    recs = [R(0), im.rec(GOFF, 1, im.VOTE, 6), R(2)]
    o = im.route(st(), recs)
    assert o.disposition == [im.ROUTED, im.DEFERRED, im.DEFERRED]
    assert o.v == {}  # the vote waits: one entry point per group and pass


def test_a_response_does_not_join_a_wave_of_another_class():
    recs = [im.rec(GOFF, 1, im.HEARTBEAT, 5), R(0)]
    assert im.route(st(), recs).disposition == [im.ROUTED, im.DEFERRED]


def test_lower_term_and_local_and_not_leader():
    recs = [R(0, term=4), R(1, term=0, type=im.SNAP_STATUS), R(2, term=5)]
    o = im.route(st(), recs)
    assert o.disposition == [im.DROP_LOWER_TERM, im.ROUTED, im.ROUTED]
    assert o.r[(1, 0)]["type"] == 4  # QE_MSG_SNAP_STATUS: a local message passes the term check
    o = im.route(st(state=0), recs)
    assert o.disposition == [im.DROP_LOWER_TERM, im.DROP_NOT_LEADER, im.DROP_NOT_LEADER]
    assert o.r == {} and o.stats[im.STAT_GROUPS] == 0
    assert o.stats[im.STAT_LOWER_TERM] == 1 and o.stats[im.STAT_NOT_LEADER] == 2


def test_two_higher_term_responses_in_one_wave():
    """The first becomes the vote row, the second is deferred (it is dropped
    as not leading once the term has risen); the equal-term member between
    them still reaches qe_progress_step, which is why it runs before
    qe_vote_step."""
    recs = [R(0, term=5, index=11), R(1, term=8), R(2, term=9)]
    o = im.route(st(), recs)
    assert o.disposition == [im.ROUTED, im.STEPDOWN, im.DEFERRED] and o.deferred == [2]
    assert o.v == {0: dict(type=im.VMSG_VOTE_RESP, frm=1, term=8, index=0, log_term=0,
                           flags=im.VMF_REJECT, src=1)}
    assert list(o.r) == [(0, 0)] and o.stats[im.STAT_STEPDOWN] == 1
    # a higher-term response behind the wave's end is no STEPDOWN
    o = im.route(st(), [R(0), R(0, term=9)])
    assert o.disposition == [im.ROUTED, im.DEFERRED] and o.v == {}


def test_tick_hup_defers_every_record_of_its_group():
    s = st(G=2)
    recs = [R(0, g=0), R(0, g=1), im.rec(GOFF, 1, im.VOTE, 6)]
    o = im.route(s, recs, tick_action=np.array([1 | 4, 4], np.uint8))
    assert o.disposition == [im.DEFERRED, im.ROUTED, im.DEFERRED]
    assert o.v == {0: dict(type=im.VMSG_HUP, frm=0, term=0, index=0, log_term=0, flags=0,
                           src=im.SRC_TICK)}
    assert o.stats[im.STAT_GROUPS] == 1
    o = im.route(s, [], tick_action=np.array([0, 1], np.uint8))  # an empty list still has HUPs
    assert list(o.v) == [1] and o.disposition == [] and o.deferred == []


def test_bad_records_take_no_part():
    """A group outside the batch (either side), an unknown type, a slot >=
    num_slots; a HUP's slot is not checked."""
    recs = [im.rec(GOFF - 1, 0, im.APP_RESP, 5), im.rec(GOFF + 1, 0, im.APP_RESP, 5),
            R(0, type=0), R(0, type=17), R(3), im.rec(GOFF, 3, im.VOTE, 5),
            im.rec(GOFF, 200, im.HUP), R(1)]
    o = im.route(st(), recs)
    assert o.disposition == [im.BAD] * 6 + [im.ROUTED, im.DEFERRED]  # not deferred, not openers
    assert o.v[0]["type"] == im.VMSG_HUP and o.v[0]["frm"] == 200
    assert o.stats[im.STAT_BAD] == o.stats[im.STAT_VIOLATIONS] == 6


def test_checksum_depends_on_position_and_disposition():
    a = im.route(st(), [R(0), R(1)]).stats[im.STAT_CHECKSUM]
    b = im.route(st(), [R(1), R(0)]).stats[im.STAT_CHECKSUM]
    c = im.route(st(state=0), [R(0), R(1)]).stats[im.STAT_CHECKSUM]
    assert len({a, b, c}) == 3
    h = im.mix64((GOFF * im.PHI) ^ im.SALT ^ (im.ROUTED << 56) ^ (im.APP_RESP << 48) ^ (2 << 40))
    assert im.route(st(), [R(2)]).stats[im.STAT_CHECKSUM] == im.mix64(h ^ 0)


def test_vectorised_record_hash_equals_the_scalar_one():
    """record_hashes (what tests/test_gpu_inbox.py sums over a list too long
    for the model) against record_hash per record on 1500 random records: group
    ids past 2^33, every disposition and every type byte, slots up to 255; and
    its sum over a routed list against route()'s STAT_CHECKSUM."""
    rng = np.random.default_rng(4242)
    n = 1500
    group = rng.integers(0, 1 << 62, n, dtype=np.uint64) | np.uint64(1 << 33)
    disp = rng.choice(list(im.ID_NAMES), n).astype(np.uint8)
    type_ = rng.integers(0, 256, n).astype(np.uint8)
    frm = rng.integers(0, 256, n).astype(np.uint8)
    got = im.record_hashes(group, disp, type_, frm)
    assert got.dtype == np.uint64 and len(set(got.tolist())) == n
    assert got.tolist() == [im.record_hash(int(group[i]), int(disp[i]), int(type_[i]),
                                           int(frm[i]), i) for i in range(n)]
    G, S = 40, 3
    s = im.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=G + 3,
                 term=rng.integers(3, 7, G), state=rng.choice([0, 1, 2, 2, 2, 3], G))
    recs = [im.rec(GOFF + int(rng.integers(0, G + 1)), int(rng.integers(0, S + 1)),
                   int(rng.integers(0, 19)), int(rng.integers(2, 8))) for _ in range(n)]
    o = im.route(s, recs)
    assert set(o.disposition) == set(im.ID_NAMES)
    a = lambda k: np.array([m[k] for m in recs], np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        total = int(np.add.reduce(im.record_hashes(a("group"), np.array(o.disposition, np.uint8),
                                                   a("type"), a("from"))))
    assert total == o.stats[im.STAT_CHECKSUM]
