"""tests/carry_model.py against the reference's network (its filter and the
addressing of send, restated in the same file), against the rule the closed
loops use on the static cluster layout, and every rule of qe_carry on its own."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import carry_model as m
from tests.inbox_model import mix64, record_hash

G, S, N = 12, 5, 3


def st_of(G=G, S=S, goff=0, stride=None):
    return SimpleNamespace(num_groups=G, group_offset=goff, num_slots=S, stride=stride or G + 2)


def static_tables(st, N=N):
    """node i of cluster c is group c * N + i and sits in slot i everywhere."""
    pg = np.full((st.num_slots, st.stride), m.PEER_NONE, np.uint64)
    pf = np.full((st.num_slots, st.stride), 0xFF, np.uint8)
    g = np.arange(st.num_groups)
    for s in range(N):
        pg[s, :st.num_groups] = st.group_offset + g - g % N + s
        pf[s, :st.num_groups] = g % N
    return pg, pf


def src_of(recs, cap=None, count=None, E=0):
    """(group, to, type[, fields]) tuples -> a source dict of `cap` records."""
    cap = len(recs) if cap is None else cap
    src = {k: np.zeros(cap, t) for k, t in (("group", np.uint64), ("to", np.uint8),
                                            ("type", np.uint8), ("term", np.uint64),
                                            ("index", np.uint64), ("log_term", np.uint64),
                                            ("commit", np.uint64), ("hint", np.uint64),
                                            ("ctx", np.uint32), ("mflags", np.uint8))}
    if E:
        src["ent_len"], src["ent_term"] = np.zeros((E, cap), np.uint32), np.zeros((E, cap), np.uint64)
    for i, r in enumerate(recs):
        src["group"][i], src["to"][i], src["type"][i] = r[:3]
        for k, v in (r[3] if len(r) > 3 else {}).items():
            if k in ("ent_len", "ent_term"):
                src[k][:len(v), i] = v
            else:
                src[k][i] = v
    src["count"] = len(recs) if count is None else count
    return src


def run(recs, st=None, tables=None, **kw):
    st = st or st_of()
    pg, pf = tables or static_tables(st)
    return m.carry(st, pg, pf, src_of(recs, **{k: kw.pop(k) for k in ("cap", "count", "E")
                                               if k in kw}), **kw)


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_reference_network(seed):
    """Seeded random lists through Network.filter + deliver and through carry(): the same
    messages in the same order.  Node ids map to groups through a peer table whose slots
    are permuted per node; fractional dropm draws and the hook are the host's `drop`."""
    rng = np.random.default_rng(900 + seed)
    st = st_of(G=12, S=6, goff=(0, 1 << 40)[seed % 2])
    pg, pf, ids = m.tables(rng, st.num_groups, st.num_slots, st.stride, st.group_offset,
                           foreign=False)
    assert (pf[:, :st.num_groups][pg[:, :st.num_groups] != m.PEER_NONE] !=
            np.nonzero(pg[:, :st.num_groups] != m.PEER_NONE)[0]).any()  # not the identity
    group_of = {int(st.group_offset + g + 1): g for g in range(st.num_groups)}
    n = 300
    g = rng.integers(0, st.num_groups, n)
    to = np.array([rng.choice(np.flatnonzero(ids[x])) for x in g])
    typ = rng.choice(m.CARRIABLE, n)
    index = rng.integers(0, 1 << 40, n)
    draws = rng.random(n)
    hook = lambda msg: msg["index"] % 7 != 0  # noqa: E731
    nw = m.Network(None, hook)
    nw.ignore(6)
    nw.ignore(13)
    a, b, c = (int(ids[0, s]) for s in np.flatnonzero(ids[0])[:3])
    nw.cut(a, b)                       # both directions, always
    nw.drop(c, a, 0.4)                 # one direction, sometimes
    nw.isolate(int(ids[5, np.flatnonzero(ids[5])[0]]), [int(x) for x in ids[5][ids[5] != 0]])
    msgs = [{"type": int(typ[i]), "from": int(st.group_offset + g[i] + 1),
             "to": int(ids[g[i], to[i]]), "index": int(index[i]), "i": i} for i in range(n)]
    # rand.Float64 is drawn for every message that is not ignored, in list order
    left = iter([draws[i] for i in range(n) if typ[i] not in (6, 13)])
    nw.rand = lambda: next(left)
    want = m.deliver(ids, group_of, nw.filter(msgs))
    # the same network as qe_carry takes it
    cut = np.zeros(st.num_groups, np.uint8)
    drop = np.zeros(n, np.uint8)
    for i, msg in enumerate(msgs):
        perc = nw.dropm.get((msg["from"], msg["to"]), 0.0)
        if perc >= 1.0:
            cut[g[i]] |= 1 << to[i]
        drop[i] = (perc < 1.0 and draws[i] < perc) or not hook(msg)
    src = src_of([(st.group_offset + g[i], to[i], typ[i], {"index": index[i]}) for i in range(n)])
    got = m.carry(st, pg, pf, src, drop, cut, (1 << 6) | (1 << 13), snap_status=False)
    loc = got.local
    assert got.count == len(want) and 0 < got.count < n
    assert [int(x) - st.group_offset for x in loc["group"]] == [w["group"] for w in want]
    assert list(loc["from"]) == [w["from"] for w in want]
    assert list(loc["type"]) == [w["type"] for w in want]
    assert list(loc["index"]) == [w["index"] for w in want]
    assert list(loc["src"]) == [w["i"] for w in want]
    assert set(np.unique(got.disposition)) == {m.LOCAL, m.LOST}


def test_hup_is_the_reference_panic():
    with pytest.raises(RuntimeError):
        m.Network(lambda: 1.0).filter([{"type": m.HUP, "from": 1, "to": 2}])
    assert list(run([(0, 1, m.HUP)]).disposition) == [m.BAD]


def test_static_layout_is_the_loops_rule():
    """receiver g - g % N + to, from = g % N (tests/test_gpu_read_states_loop.py)."""
    rng = np.random.default_rng(5)
    st = st_of(G=30, S=3, goff=7)
    g, to = rng.integers(0, 30, 200), rng.integers(0, 3, 200)
    got = m.carry(st, *static_tables(st), src_of([(7 + g[i], to[i], 4) for i in range(200)]))
    assert got.count == 200 and (got.disposition == m.LOCAL).all()
    assert np.array_equal(got.local["group"], (7 + g - g % N + to).astype(np.uint64))
    assert np.array_equal(got.local["from"], (g % N).astype(np.uint8))


@pytest.mark.parametrize("t", [0, 7, 8, 9, 16, 17, 31, 32, 200, 255])
def test_bad_type(t):
    r = run([(0, 1, t)])
    assert list(r.disposition) == [m.BAD] and r.count == 0 and not len(r.remote)
    assert r.stats[m.STAT_BAD] == r.stats[m.STAT_VIOLATIONS] == 1


def test_bad_causes():
    st = st_of(goff=100)
    pg, pf = static_tables(st)
    pf[2, 4] = S           # group 4's slot at its peer is no slot
    pf[1, 5] = 0xFF
    pg[1, 3] = 5000        # outside the batch: its peer_from is not looked at
    pf[1, 3] = 0xFF
    r = m.carry(st, pg, pf, src_of([
        (99, 0, 1), (100 + G, 0, 1), (1 << 63, 0, 1),      # group outside the batch
        (100, S, 1), (100, 255, 1),                       # to >= S
        (100, 3, 1), (100, 4, 1),                         # a slot with no peer
        (104, 2, 1), (105, 1, 1),                         # in the batch, peer_from >= S
        (103, 1, 1), (100, 1, 1)]))                       # REMOTE, LOCAL
    assert list(r.disposition) == [m.BAD] * 9 + [m.REMOTE, m.LOCAL]
    assert list(r.remote) == [9] and r.count == 1 and list(r.local["src"]) == [10]


def test_each_lost_cause_and_one_way_cut():
    cut = np.zeros(G, np.uint8)
    cut[0] = 1 << 1            # 0 -> slot 1 (group 1) is down; 1 -> slot 0 is not
    drop = np.array([0, 0, 0, 1, 0], np.uint8)
    recs = [(0, 1, 4), (1, 0, 4), (2, 0, 6), (2, 0, 4), (2, 1, 4)]
    r = run(recs, cut=cut, drop=drop, ignore=1 << 6)
    assert list(r.disposition) == [m.LOST, m.LOCAL, m.LOST, m.LOST, m.LOCAL]
    assert list(r.local["src"]) == [1, 4] and list(r.local["group"]) == [0, 1]
    assert r.stats[m.STAT_LOST] == 3 and r.stats[m.STAT_LOCAL] == 2
    # BAD goes before LOST: a dropped record with a bad type is BAD
    assert list(run([(0, 1, 9)], drop=np.ones(1, np.uint8)).disposition) == [m.BAD]
    # a 16-bit mask row
    st = st_of(S=12)
    pg, pf = static_tables(st)
    pg[11, 0], pf[11, 0] = 3, 4
    cut16 = np.zeros(G, np.uint16)
    cut16[0] = 1 << 11
    r = m.carry(st, pg, pf, src_of([(0, 11, 1), (0, 1, 1)]), cut=cut16)
    assert list(r.disposition) == [m.LOST, m.LOCAL]


def test_remote_gets_no_status():
    st = st_of()
    pg, pf = static_tables(st)
    pg[1, 0] = 77777
    r = m.carry(st, pg, pf, src_of([(0, 1, m.SNAP), (0, 2, m.SNAP)]))
    assert list(r.disposition) == [m.REMOTE, m.LOCAL] and list(r.remote) == [0]
    assert list(r.local["type"]) == [m.SNAP, m.SNAP_STATUS] and list(r.local["src"]) == [1, 1]
    assert r.stats[m.STAT_SNAP_STATUS] == 1 and r.stats[m.STAT_REMOTE] == 1


def test_status_sits_behind_its_snap_and_reject_stands_in_its_place():
    f = dict(term=5, index=40, log_term=3, commit=9, hint=1, ctx=2, mflags=3)
    recs = [(4, 0, 4, f), (4, 2, m.SNAP, f), (7, 0, m.SNAP, f), (4, 0, 1, f)]
    r = run(recs, drop=np.array([0, 0, 1, 0], np.uint8))
    loc = r.local
    assert list(r.disposition) == [m.LOCAL, m.LOCAL, m.LOST, m.LOCAL] and r.count == 5
    assert list(loc["type"]) == [4, m.SNAP, m.SNAP_STATUS, m.SNAP_STATUS_REJECT, 1]
    assert list(loc["group"]) == [3, 5, 4, 7, 3]     # receiver, receiver, SENDER, SENDER, receiver
    assert list(loc["from"]) == [1, 1, 2, 0, 1]      # a status comes `from` the slot it was sent to
    assert list(loc["src"]) == [0, 1, 1, 2, 3]
    for k, v in f.items():                           # a status record: term 0, every field 0
        assert list(loc[k]) == [v, v, 0, 0, v], k
    assert r.stats[m.STAT_SNAP_STATUS] == 2 and r.stats[m.STAT_GROUPS] == 5
    # the flag off: no status records
    r = run(recs, drop=np.array([0, 0, 1, 0], np.uint8), snap_status=False)
    assert list(r.local["type"]) == [4, m.SNAP, 1] and r.stats[m.STAT_SNAP_STATUS] == 0
    assert list(r.disposition) == [m.LOCAL, m.LOCAL, m.LOST, m.LOCAL]


def test_count_clips_and_records_behind_n_are_ignored():
    recs = [(0, 1, 4), (1, 0, 4), (2, 0, 4)]
    r = run(recs, cap=3, count=2)
    assert r.n == 2 and len(r.disposition) == 2 and r.count == 2
    r = run(recs, cap=3, count=99)
    assert r.n == 3 and r.count == 3


def test_truncation_base_and_pitch():
    recs = [(g, (g + 1) % N, m.SNAP, {"index": 10 + g, "ent_len": [g + 1], "ent_term": [g + 2]})
            for g in range(6)]
    r = run(recs, E=1, msg_runs_out=3)
    assert r.count == 12 and r.local["ent_len"].shape == (3, 12)
    assert list(r.local["ent_len"][0]) == [1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 0]
    assert not r.local["ent_len"][1:].any() and not r.local["ent_term"][1:].any()  # E_in <= j < E_out
    cap, base, pitch = 9, 4, 11
    arr = {"index": np.full(cap, 0xEE, np.uint64), "ent_len": np.full(3 * pitch, 0xEE, np.uint32),
           "src": None}
    m.place(r, arr, base, cap, pitch)
    assert list(arr["index"]) == [0xEE] * 4 + [10, 0, 11, 0, 12]      # five of twelve fit
    e = arr["ent_len"].reshape(3, pitch)
    assert list(e[0]) == [0xEE] * 4 + [1, 0, 2, 0, 3, 0xEE, 0xEE]
    assert list(e[1]) == [0xEE] * 4 + [0] * 5 + [0xEE, 0xEE]
    assert r.stats[m.STAT_GROUPS] == 12                               # asked for, not written
    short = np.full(cap, 0xEE, np.uint64)
    m.place(run(recs[:1], E=1), {"index": short}, base, cap, pitch)
    assert list(short) == [0xEE] * 4 + [10, 0] + [0xEE] * 3           # nothing past base + count


def test_checksum_depends_on_position_and_disposition():
    a = run([(0, 1, 4), (1, 0, 5)])
    b = run([(1, 0, 5), (0, 1, 4)])
    assert a.stats[m.STAT_CHECKSUM] != b.stats[m.STAT_CHECKSUM]       # position
    c = run([(0, 1, 4), (1, 0, 5)], drop=np.array([1, 0], np.uint8))
    assert a.stats[m.STAT_CHECKSUM] != c.stats[m.STAT_CHECKSUM]       # disposition
    # the scalar form of the header, under qe_carry's own salt
    M = (1 << 64) - 1

    def term(g, d, t, to, i):
        return mix64(mix64(((g * 0x9E3779B97F4A7C15) & M) ^ m.SALT ^ (d << 56) ^ (t << 48) ^
                           (to << 40)) ^ i)

    assert int(a.stats[m.STAT_CHECKSUM]) == (term(0, 1, 4, 1, 0) + term(1, 1, 5, 0, 1)) & M
    assert term(0, 1, 4, 1, 0) != record_hash(0, 1, 4, 1, 0)  # (qe_inbox's salt)


def test_cases_cover_every_value_the_issue_names():
    cs = m.cases()
    big = [c for c in cs if c.want.n >= 63]
    assert {c.want.n for c in cs} >= set(m.LENGTHS)
    assert {c.st.num_groups for c in big} == {9, 69} and {c.st.num_slots for c in big} == {3, 9}
    assert {c.st.group_offset for c in big} == {0, 1 << 40}
    assert {(0 if c.src.get("ent_len") is None else len(c.src["ent_len"]), c.E_out)
            for c in cs} == {(0, 0), (1, 1), (0, 4), (4, 4)}
    assert {c.form for c in big} == {"outbox", "replies"} and {c.stats for c in big} == {True, False}
    assert all(c.st.stride == c.st.num_groups + 3 for c in cs)
    for n in m.LENGTHS:
        assert {c.form for c in cs if c.want.n == n and c.src["count"] == n} == {"outbox", "replies"}
    assert any((c.src["term"] >> np.uint64(63)).any() for c in big)
    assert any(c.src["count"] < len(c.src["group"]) for c in cs)
    assert any(c.src["count"] > len(c.src["group"]) for c in cs)
