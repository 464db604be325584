"""qe_inbox on the device against tests/inbox_model.py on random lists: every
row of the four families, the source positions, the dispositions, the deferred
list with its count and the statistics.  Every output is prefilled with the
sentinel of tests/test_gpu_cluster.py and whatever the rules do not write must
keep it; f->term and f->state must be byte-identical before and after; the
same list routed twice must give identical bytes.

The shapes: G = 1 (one lane), 63 (a ragged tile), 65 (a ragged second tile) and
4097 (a second 4096-chunk of the init pass); S = 1, 3, 9 (16-bit masks' side of
8) and 16; msg_runs 0, 1, 4; n = 0, 1, 63, 64, 65 (the record tile's edges) and
4097 (a second chunk of qe_collect's scan); stride = G + 3; group_offset 2^33;
4096 records aimed at two groups (every atomic of a tile on two words); records
outside the batch on both sides; with and without tick_action, ctx, flags and
the *_src rows; receiver terms 3..6 against message terms one below, equal, one
above and 0, and every state, so that all five preamble outcomes occur.

test_route_waves_walk is the one list long enough for the routing pass's capped
grid (with statistics, 8 blocks per CU): its waves walk two and three tiles and
carry their counters across them."""
import zlib
from collections import Counter

import numpy as np
import pytest
import torch

from tests import inbox_model as im

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x0E0E0E0E0E0E0E0E
GOFF = 1 << 33
NP = {torch.int64: np.uint64, torch.int32: np.uint32, torch.int16: np.uint16, torch.uint8: np.uint8}
TYPES = list(range(0, 19))  # 0, 17 and 18 are no QE_IMSG_*
#            none  F     S     F     R x 7                          V x 6              none
TYPE_P = np.array([1, 3, 2, 3] + [8] * 7 + [2, 2, 2, 2, 1, 1] + [1, 1], float)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def host(t):
    return t.cpu().numpy().view(NP[t.dtype])


def sentinel(t):
    if t is not None:
        t.view(torch.uint8).fill_(SENT & 0xFF)


def kept(a):
    """Every byte of `a` is still the sentinel's."""
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT & 0xFF).all())


def random_list(rng, G, S, E, n, mode):
    groups = np.array([0, G - 1]) if mode == "two" else np.arange(G)
    recs = []
    for i in range(n):
        g = GOFF + int(rng.choice(groups))
        u = rng.random()
        if u < 0.02:
            g = GOFF - 1 - int(rng.integers(0, 3))       # below the batch
        elif u < 0.04:
            g = GOFF + G + int(rng.integers(0, 3))       # above it
        t = int(rng.choice(TYPES, p=TYPE_P / TYPE_P.sum()))
        frm = int(rng.integers(0, S + 1)) if rng.random() < 0.1 else int(rng.integers(0, S))
        if t == im.HUP and rng.random() < 0.5:
            frm = 200
        ents = [(int(rng.integers(0, 9)), int(rng.integers(1, 1 << 40))) for _ in range(E)]
        recs.append(im.rec(g, frm, t, 0, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62)),
                           int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62)),
                           int(rng.integers(0, 1 << 32)), int(rng.integers(0, 4)), ents))
    if n >= 2 and mode != "two":
        recs[n // 2]["group"] = GOFF + G                 # one outside for sure
    return recs


def set_terms(rng, recs, rterm, G):
    for m in recs:
        g = m["group"] - GOFF
        base = int(rterm[g]) if 0 <= g < G else 4
        m["term"] = base + int(rng.choice([-1, 0, 0, 0, 1, -base]))


def arrays(recs, E, ctx, flags):
    u64 = lambda k: np.array([m[k] for m in recs], np.uint64)  # noqa: E731
    a = {k: u64(k) for k in ("group", "term", "index", "log_term", "commit", "hint")}
    a["from"] = np.array([m["from"] for m in recs], np.uint8)
    a["type"] = np.array([m["type"] for m in recs], np.uint8)
    if ctx:
        a["ctx"] = np.array([m["ctx"] for m in recs], np.uint32)
    if flags:
        a["flags"] = np.array([m["flags"] for m in recs], np.uint8)
    if E:
        a["ent_len"] = np.array([[m["ents"][j][0] for m in recs] for j in range(E)], np.uint32)
        a["ent_term"] = np.array([[m["ents"][j][1] for m in recs] for j in range(E)], np.uint64)
    return a


class Rows:
    """The four row families (fresh, sentinel-filled) and one routed pass."""

    def __init__(self, e, ps, fol, E, o):
        self.lm, self.sm = e.LeaderMsgs(ps, E), e.SnapMsgs(ps)
        self.vm, self.pm = e.VoteMsgs(ps), e.PeerMsgs(ps, outputs=False)
        if o["ctx"]:
            self.pm.set_read_ctx(ps, np.zeros(ps.S * ps.stride, np.uint32))
        if not o["flags"]:
            self.vm.flags = None
        self.f = dict(type=self.lm.type, frm=self.lm.from_, term=self.lm.term, index=self.lm.index,
                      log_term=self.lm.log_term, commit=self.lm.commit)
        self.s = dict(type=self.sm.type, frm=self.sm.from_, term=self.sm.term,
                      snap_index=self.sm.snap_index, snap_term=self.sm.snap_term)
        self.v = dict(type=self.vm.type, frm=self.vm.from_, term=self.vm.term, index=self.vm.index,
                      log_term=self.vm.log_term, flags=self.vm.flags)
        self.r = dict(type=self.pm.type, index=self.pm.index, hint=self.pm.reject_hint,
                      log_term=self.pm.log_term, ctx=self.pm.read_ctx)
        for d in (self.f, self.s, self.v, self.r):
            for t in d.values():
                sentinel(t)
        sentinel(self.lm.ent_len), sentinel(self.lm.ent_term)

    def tensors(self, ib):
        out = [t for d in (self.f, self.s, self.v, self.r) for t in d.values() if t is not None]
        out += [t for t in (self.lm.ent_len, self.lm.ent_term, ib.f_src, ib.s_src, ib.v_src,
                            ib.r_src, ib.disposition, ib.deferred, ib.deferred_count)
                if t is not None]
        return out


def fresh_inbox(e, ps, E, o, a, n):
    ib = e.Inbox(ps, n + 5, E, ctx=o["ctx"], flags=o["flags"], src=o["src"])
    ib.load_host(**a)
    for t in (ib.disposition, ib.deferred, ib.deferred_count, ib.f_src, ib.s_src, ib.v_src,
              ib.r_src):
        sentinel(t)
    return ib


def check_family(name, rows, want, src, G, opt=()):
    """rows: field -> tensor [G]; want: g -> the model's row."""
    ty = host(rows["type"])
    has = np.zeros(G, bool)
    has[list(want)] = True
    np.testing.assert_array_equal(ty, [want[g]["type"] if g in want else 0 for g in range(G)],
                                  err_msg=name + "_type")
    fields = dict(rows, src=src)
    for k, t in fields.items():
        if k == "type" or t is None:
            assert k == "type" or k in opt + ("src",), (name, k)
            continue
        got = host(t)
        exp = np.array([want[g][k] for g in sorted(want)], np.uint64).astype(got.dtype)
        np.testing.assert_array_equal(got[has], exp, err_msg=f"{name}_{k}")
        assert kept(got[~has]), f"{name}_{k}: written where {name}_type is 0"


ALL = dict(tick=True, ctx=True, flags=True, src=True)
NONE = dict(tick=False, ctx=False, flags=False, src=False)
#        G     S   E  n     mode    options
CASES = [
    (1,    1,  0, 0,    "rand", ALL),
    (1,    3,  1, 1,    "rand", NONE),
    (1,    16, 4, 65,   "rand", dict(ALL, tick=False)),
    (63,   1,  1, 63,   "rand", ALL),
    (63,   3,  4, 64,   "rand", dict(NONE, src=True)),
    (63,   9,  0, 65,   "rand", dict(ALL, flags=False)),
    (63,   16, 4, 4097, "rand", ALL),
    (65,   3,  4, 4097, "rand", dict(ALL, tick=False)),
    (65,   9,  1, 65,   "rand", dict(NONE, tick=True)),
    (65,   16, 0, 64,   "rand", dict(ALL, ctx=False)),
    (65,   3,  1, 4096, "two",  ALL),
    (65,   9,  4, 4096, "two",  dict(NONE, ctx=True)),
    (4097, 1,  1, 4097, "rand", ALL),
    (4097, 3,  4, 4097, "rand", NONE),
    (4097, 9,  0, 63,   "rand", ALL),
    (4097, 16, 4, 0,    "rand", ALL),
    (4097, 5,  1, 1,    "rand", dict(ALL, tick=False)),
]


@pytest.mark.parametrize("G,S,E,n,mode,o", CASES)
def test_inbox_matches_model(eng, G, S, E, n, mode, o):
    e = eng
    rng = np.random.default_rng(zlib.crc32(repr((G, S, E, n, mode, sorted(o.items()))).encode()))
    st = G + 3
    rterm = rng.integers(3, 7, G).astype(np.uint64)
    state = rng.choice([0, 1, 2, 2, 2, 3], G).astype(np.uint8)
    recs = random_list(rng, G, S, E, n, mode)
    set_terms(rng, recs, rterm, G)
    tick = None
    if o["tick"]:
        tick = (rng.integers(0, 8, G) & np.where(rng.random(G) < 0.2, 7, 6)).astype(np.uint8)
        if mode == "two":
            tick[[0, G - 1]] &= 6
    # ---- the model ----
    mst = im.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=st, term=rterm, state=state)
    want = im.route(mst, recs, tick, E)
    if n >= 4096 and G in (63, 65) and mode == "rand":  # enough records per group
        assert set(want.disposition) == set(im.ID_NAMES), Counter(want.disposition)
        assert any(len(w) >= 3 for w in want.waves.values())
    # ---- the device, twice ----
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF, stride=st)
    fol = e.Follower(ps)
    fol.load_host(term=rterm, state=state)
    before = (fol.term.clone(), fol.state.clone())
    tick_t = None if tick is None else torch.from_numpy(tick).to(DEV)
    a = arrays(recs, E, o["ctx"], o["flags"])
    runs = []
    for _ in range(2):
        ib, rows = fresh_inbox(e, ps, E, o, a, n), Rows(e, ps, fol, E, o)
        stats = e.stats_buffer(DEV)
        e.inbox(ps, fol, ib, rows.lm, rows.sm, rows.vm, rows.pm, tick_action=tick_t, stats=stats)
        folded = host(e.stats_reduce(stats))
        torch.cuda.synchronize()
        runs.append([t.clone() for t in rows.tensors(ib)] + [torch.from_numpy(folded.copy())])
    for x, y in zip(*runs):
        assert torch.equal(x, y), "two runs of one list differ"
    assert torch.equal(fol.term, before[0]) and torch.equal(fol.state, before[1])
    # ---- the per-group families ----
    src = lambda k: getattr(ib, k) if o["src"] else None  # noqa: E731
    check_family("f", rows.f, want.f, src("f_src"), G)
    check_family("s", rows.s, want.s, src("s_src"), G)
    check_family("v", rows.v, want.v, src("v_src"), G, opt=("flags",))
    if E:
        el, et = host(rows.lm.ent_len).reshape(E, st), host(rows.lm.ent_term).reshape(E, st)
        app = np.zeros(st, bool)
        for g, r in want.f.items():
            if r["ents"] is not None:
                app[g] = True
                np.testing.assert_array_equal(el[:, g], [x[0] for x in r["ents"]])
                np.testing.assert_array_equal(et[:, g], [x[1] for x in r["ents"]])
        assert kept(el[:, ~app]) and kept(et[:, ~app]), "entry rows written for no MsgApp"
    # ---- the response rows [S][stride] ----
    rt = host(rows.r["type"]).reshape(S, st)
    exp = np.zeros((S, G), np.uint8)
    for (s, g), r in want.r.items():
        exp[s, g] = r["type"]
    np.testing.assert_array_equal(rt[:, :G], exp, err_msg="r_type")
    assert kept(rt[:, G:]), "r_type: a pad column was written"
    fields = dict(rows.r, src=src("r_src"))
    for k, t in fields.items():
        if k == "type" or t is None:
            continue
        got = host(t).reshape(S, st)
        has = np.zeros((S, st), bool)
        for (s, g), r in want.r.items():
            has[s, g] = True
            assert int(got[s, g]) == r[k], ("r_" + k, s, g)
        assert kept(got[~has]), f"r_{k}: written where r_type is 0"
    # ---- per record ----
    disp = host(ib.disposition)
    np.testing.assert_array_equal(disp[:n], want.disposition, err_msg="disposition")
    assert kept(disp[n:])
    count = int(host(ib.deferred_count)[0])
    assert count == len(want.deferred)
    dl = host(ib.deferred)
    np.testing.assert_array_equal(dl[:count], want.deferred, err_msg="deferred")
    assert kept(dl[count:])
    d2, l2 = ib.results()
    np.testing.assert_array_equal(d2, want.disposition)
    np.testing.assert_array_equal(l2, want.deferred)
    for i in range(16):
        assert int(folded[i]) == want.stats.get(i, 0), ("stat", i)
    # ---- the next pass's list, gathered on the device ----
    nxt = ib.gather_deferred(e.Inbox(ps, n + 5, E, ctx=o["ctx"], flags=o["flags"], src=False))
    assert nxt.n == count
    sub = arrays([recs[i] for i in want.deferred], E, o["ctx"], o["flags"])
    for k, v in sub.items():
        t = getattr(nxt, "from_" if k == "from" else k)
        np.testing.assert_array_equal(host(t)[: v.size], v.reshape(-1), err_msg="gathered " + k)


def three_chunk_list(S, E):
    """tests/walk.py's three_chunks() as an inbox list over leaders at term 4:
    a MsgApp opens each hot group (ROUTED, a non-R opener closes its group),
    responses and votes follow into the hot groups (DEFERRED), and the lone
    records are of every class, the responses one term below, equal and one
    above (DROP_LOWER_TERM, ROUTED, STEPDOWN: never DEFERRED)."""
    from tests import walk
    G, role, group = walk.three_chunks()
    lone = [im.APP, im.HEARTBEAT, im.SNAP, im.VOTE, im.APP_RESP, im.HEARTBEAT_RESP, im.HUP]
    hot = [im.APP_RESP, im.VOTE, im.HEARTBEAT_RESP, im.APP]
    recs = []
    for i, (ro, g) in enumerate(zip(role.tolist(), group.tolist())):
        t = {walk.OPEN: im.APP, walk.HOT: hot[i % 4], walk.LONE: lone[i % 7], walk.OUT: im.APP}[ro]
        term = 3 + i % 3 if ro == walk.LONE and im.cls_of(t) == im.R_CLS else 4
        recs.append(im.rec(GOFF + g, i % S, t, term, 1000 + i, 3, 900 + i, i, i, i % 4,
                           [(1 + i % 7, 4)] * E))
    return G, group, recs


@pytest.mark.parametrize("with_stats", [False, True])
def test_deferred_positions_over_three_chunks(eng, with_stats):
    """The deferred list past its second 4096-record chunk (tests/walk.py
    three_chunks: a chunk whose base comes from two predecessors, a chunk and
    tiles with no deferred record, a full tile, the ragged last chunk of one
    record): the dispositions, the count, every deferred position and the
    poison behind them against the model, with statistics the folded counters
    and the checksum too."""
    from tests import walk
    e, S, E, o = eng, 3, 1, NONE
    G, group, recs = three_chunk_list(S, E)
    n, st = len(recs), G + 3
    rterm, state = np.full(G, 4, np.uint64), np.full(G, im.ST_LEADER, np.uint8)
    want = im.route(im.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=st, term=rterm,
                             state=state), recs, None, E)
    walk.check_three_chunks(want.deferred, group)
    assert set(want.disposition) == set(im.ID_NAMES) - {im.DROP_NOT_LEADER}
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF, stride=st)
    fol = e.Follower(ps)
    fol.load_host(term=rterm, state=state)
    ib, rows = fresh_inbox(e, ps, E, o, arrays(recs, E, o["ctx"], o["flags"]), n), Rows(e, ps, fol, E, o)
    stats = e.stats_buffer(DEV) if with_stats else None
    e.inbox(ps, fol, ib, rows.lm, rows.sm, rows.vm, rows.pm, stats=stats)
    disp = host(ib.disposition)
    np.testing.assert_array_equal(disp[:n], want.disposition, err_msg="disposition")
    assert kept(disp[n:])
    count = int(host(ib.deferred_count)[0])
    assert count == len(want.deferred)
    dl = host(ib.deferred)
    np.testing.assert_array_equal(dl[:count], want.deferred, err_msg="deferred")
    assert kept(dl[count:])
    if with_stats:
        folded = host(e.stats_reduce(stats))
        for i in range(16):
            assert int(folded[i]) == want.stats.get(i, 0), ("stat", i)


def test_route_waves_walk(eng):
    """A list of (2 * cap + 2) tiles and 21 records, cap = the wave count of
    the routing pass's capped grid: with statistics every wave of k_inbox_p3
    walks two tiles, two walk three and the last tile is ragged.  The same list
    without statistics takes a wave per tile (what the model tests pin at small
    n).  Between the two calls every row, source position, disposition and the
    deferred list must be the same bytes, and the folded counters, carried by
    each wave over its walk, must be what the outputs determine: the
    per-disposition counters from the disposition array, QE_STAT_GROUPS the
    distinct groups with a ROUTED record, QE_STAT_CHECKSUM the sum of
    tests/inbox_model.py's record hash (record_hashes, pinned to the scalar one
    in tests/test_inbox_model.py).  The records are generated on the device:
    about two per group, 4% outside the batch, types that are none and slots
    out of range, terms one below, equal, one above and 0."""
    from tests import walk
    from tests.test_gpu_outbox import DeviceRandom
    e = eng
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    n = walk.walk_groups(cus)
    G, S, E = n // 2 + 3, 5, 1
    o = dict(ALL, tick=False)
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF, stride=G + 3)
    fol = e.Follower(ps)
    per_group, rnd = DeviceRandom(G, 0x1B0C), DeviceRandom(n, 0x1B0D)
    fol.term.copy_(per_group.ints(3, 7))
    fol.state.copy_(torch.tensor([0, 1, 2, 2, 2, 3], dtype=torch.uint8, device=DEV)[per_group.ints(0, 6)])
    g = rnd.ints(0, G)
    u = torch.rand(n, generator=rnd.gen, device=DEV)
    inside = (u >= 0.04)
    gid = torch.where(inside, GOFF + g, torch.where(u < 0.02, GOFF - 1 - rnd.ints(0, 3),
                                                    GOFF + G + rnd.ints(0, 3)))
    base = torch.where(inside, fol.term[g], torch.full_like(g, 4))
    delta = torch.tensor([-1, 0, 0, 0, 1], device=DEV)[rnd.ints(0, 5)]
    term = torch.where(rnd.hit(1 / 6), torch.zeros_like(base), base + delta)
    p = torch.tensor(TYPE_P, dtype=torch.float32, device=DEV)
    ty = torch.multinomial(p, n, replacement=True, generator=rnd.gen).to(torch.uint8)
    frm = torch.where(rnd.hit(0.02), torch.full_like(g, S), rnd.ints(0, S)).to(torch.uint8)
    big = lambda: rnd.ints(0, 1 << 62)  # noqa: E731
    rec = dict(group=gid, from_=frm, type=ty, term=term, index=big(), log_term=big(),
               commit=big(), hint=big(), ctx=rnd.ints(0, 1 << 31, torch.int32),
               flags=rnd.ints(0, 4, torch.uint8), ent_len=rnd.ints(0, 9, torch.int32),
               ent_term=rnd.ints(1, 1 << 40))  # (E = 1: the run rows are [1][n])
    runs = []
    for stats in (None, e.stats_buffer(DEV)):
        ib = e.Inbox(ps, n, E, ctx=o["ctx"], flags=o["flags"], src=o["src"])
        for k, t in rec.items():
            getattr(ib, k).copy_(t)
        ib.n = n
        for t in (ib.disposition, ib.deferred, ib.deferred_count, ib.f_src, ib.s_src, ib.v_src,
                  ib.r_src):
            sentinel(t)
        rows = Rows(e, ps, fol, E, o)
        e.inbox(ps, fol, ib, rows.lm, rows.sm, rows.vm, rows.pm, stats=stats)
        runs.append(rows.tensors(ib))
    names = [k for d in "fsvr" for k, t in getattr(rows, d).items() if t is not None]
    assert len(runs[0]) == len(runs[1]) > len(names)
    for i, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), ("with and without statistics differ", i, names[i:i + 1])
    # ---- the counters against the outputs ----
    folded = host(e.stats_reduce(stats))
    disp = host(ib.disposition)
    cnt = np.bincount(disp, minlength=256)
    assert all(cnt[d] > 0 for d in im.ID_NAMES), {im.ID_NAMES[d]: int(cnt[d]) for d in im.ID_NAMES}
    assert int(cnt.sum()) == n == sum(int(cnt[d]) for d in im.ID_NAMES)
    for d, stat in im.BY_DISPOSITION.items():
        assert int(folded[stat]) == int(cnt[d]), ("stat", im.ID_NAMES[d])
    assert int(folded[im.STAT_VIOLATIONS]) == int(cnt[im.BAD])
    gh = host(gid)
    assert int(folded[im.STAT_GROUPS]) == np.unique(gh[disp == im.ROUTED]).size
    with np.errstate(over="ignore"):
        csum = int(np.add.reduce(im.record_hashes(gh, disp, host(ty), host(frm))))
    assert int(folded[im.STAT_CHECKSUM]) == csum
    count = int(host(ib.deferred_count)[0])
    np.testing.assert_array_equal(host(ib.deferred)[:count], np.flatnonzero(disp == im.DEFERRED))
