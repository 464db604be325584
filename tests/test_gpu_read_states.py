"""qe_read_note / qe_read_states on the GPU: the reference's ReadIndex tests
with the answers themselves checked (ReadState{Index, RequestCtx} and
MsgReadIndexResp{To, Index}, not only a released count), a random
differential against the row-level model (tests/read_states_model.py, itself
held against read_only.go in tests/test_read_states_model.py), the extremes of
the tile (one group with 255 records beside groups with none, a tile of
TERM_COMMIT + immediate answers, nothing at all) and capacity cuts."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import read_states_model as rsm
from tests.leader_round_scenarios import (POSTPONED, QUEUED, RESPOND, _heartbeat_round,
                                          _leader_after_hup, _peer, _propose)
from tests.progress_scenarios import initial_arrays
from tests.test_gpu_progress import (DEV, EXTRAS, GpuBackend, load_msgs, random_msgs,
                                     random_state, to_device)

pytestmark = pytest.mark.gpu
STATE, RESP, TERM_COMMIT = _lib.QE_RS_STATE, _lib.QE_RS_RESP, _lib.QE_RS_TERM_COMMIT
NONE = 0xFF
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(DEV)


# ---- the reference's tests, the answers checked ----

class Backend(GpuBackend):
    """The one-group backend of tests/leader_round_scenarios.py with the
    request book: read_index notes what it queued, answers() lists what the
    last call (a step or a read_index) answered."""

    def load(self, *a, **kw):
        super().load(*a, **kw)
        self.book = self.eng.ReadBook(self.ps)
        self.rs = self.eng.ReadStates(self.ps, 8)
        self.msgs = self.ri = None

    def step(self, t, idx, hint, lt, ctx=None):
        msgs = load_msgs(self.eng, self.ps, t, idx, hint, lt)
        msgs.set_read_ctx(self.ps, ctx)
        self.eng.progress_step(self.ps, msgs)
        self.msgs, self.ri = msgs, None
        return {"sent": int(msgs.sent[0]), "read_released": int(msgs.read_released[0]),
                "term_commit": int(msgs.term_commit[0]),
                "term_commit_index": int(msgs.term_commit_index[0])}

    def read_index(self, lease_based=False, key=None, frm=None, at=None):
        """-> (result, ctx, index); frm: req.From as a slot (None: local); at:
        the index the request is noted at (None: the one the call returned)."""
        req = torch.ones(1, dtype=torch.uint8, device=DEV)
        k = None if key is None else torch.tensor([key], dtype=torch.int64, device=DEV)
        f = None if frm is None else torch.tensor([frm], dtype=torch.uint8, device=DEV)
        r, c, i = self.eng.read_index(self.ps, req, lease_based, key=k)
        noted = i if at is None else torch.tensor([at], dtype=torch.int64, device=DEV)
        self.eng.read_note(self.ps, self.book, r, c, noted, f)
        self.msgs, self.ri = None, (r, c, i, f, k)
        return int(r[0]), int(c[0]) & M32, int(i[0])

    def answers(self):
        """[(kind, to, ctx, index, key)] of the last call."""
        self.eng.read_states(self.ps, self.book, self.rs, msgs=self.msgs, ri=self.ri)
        count, r = self.rs.records()
        assert count <= self.rs.capacity and (r["group"] == 0).all()
        return [(int(r["kind"][n]), int(r["to"][n]), int(r["ctx"][n]), int(r["index"][n]),
                 int(r["key"][n])) for n in range(count)]


@pytest.mark.parametrize("forwarded", [False, True])
def test_read_only_option_safe(eng, forwarded):
    """TestReadOnlyOptionSafe (raft/raft_test.go:2177-2229): the table of
    :2200-2205, wri = 11, 21, ..., 61 with wctx = ctx1..ctx6, and the checks of
    :2216-2226: one ReadState{Index: wri, RequestCtx: wctx} each.  The leader's
    side: with the request local (the scenario of leader_round_scenarios) the
    record is a QE_RS_STATE; `forwarded` takes the table's sm column (a, b, c,
    a, b, c) as req.From: b's and c's requests reach leader a as MsgReadIndex
    from 2 and 3 and are answered by a MsgReadIndexResp{To, Index: wri} (the
    ReadState is then b's and c's own, :2219)."""
    be, S = Backend(eng), 3
    sc = _leader_after_hup(S)
    be.load(sc, initial_arrays(sc))
    table = [(0, 11, 0xC1), (1, 21, 0xC2), (2, 31, 0xC3), (0, 41, 0xC4), (1, 51, 0xC5),
             (2, 61, 0xC6)]
    for sm, wri, wctx in table:
        for _ in range(10):
            _propose(be, S, (1, 2))
        res, ctx, index = be.read_index(key=wctx, frm=sm if forwarded else None)
        assert (res, index) == (QUEUED, wri)
        assert be.answers() == []  # queued: no answer yet
        out = _heartbeat_round(be, S, (1,), ctx=ctx)  # b's response: a quorum with a's own ack
        assert out["read_released"] == 1
        local = not forwarded or sm == 0
        assert be.answers() == [(STATE if local else RESP, NONE if local else sm, ctx, wri, wctx)]
        out = _heartbeat_round(be, S, (2,), ctx=ctx)  # c's late response: recvAck finds nothing
        assert out["read_released"] == 0 and be.answers() == []


def test_read_only_with_learner(eng):
    """TestReadOnlyWithLearner (raft_test.go:2231-2278; the table :2253-2256:
    wri = 11, 21, 31, 41, wctx ctx1..ctx4; checks :2267-2277): IsSingleton
    answers at once -- rule 5."""
    be, S = Backend(eng), 2
    sc = _leader_after_hup(S)
    be.load(sc, initial_arrays(sc), inc=0b01)
    for n, wri in enumerate([11, 21, 31, 41]):
        for _ in range(10):
            _propose(be, S, (1,))
        res, _, index = be.read_index(key=0xC1 + n)
        assert (res, index) == (RESPOND, wri)
        assert be.answers() == [(STATE, NONE, 0, wri, 0xC1 + n)]


def test_read_only_option_lease(eng):
    """TestReadOnlyOptionLease (raft_test.go:2282-2337; the table :2311-2316,
    wri = 11, ..., 61; checks :2327-2334): ReadOnlyLeaseBased answers at once
    -- rule 5; sm = b, c there: the forwarded request's answer is a
    MsgReadIndexResp."""
    be, S = Backend(eng), 3
    sc = _leader_after_hup(S)
    be.load(sc, initial_arrays(sc))
    for n, (sm, wri) in enumerate([(0, 11), (1, 21), (2, 31), (0, 41), (1, 51), (2, 61)]):
        for _ in range(10):
            _propose(be, S, (1, 2))
        res, _, index = be.read_index(lease_based=True, key=0xC1 + n, frm=sm)
        assert (res, index) == (RESPOND, wri)
        assert be.answers() == [(STATE, NONE, 0, wri, 0xC1 + n) if sm == 0 else
                                (RESP, sm, 0, wri, 0xC1 + n)]


def test_raft_frees_read_only_mem(eng):
    """TestRaftFreesReadOnlyMem (raft_test.go:1359-1403): MsgReadIndex{From: 2}
    (:1369) on leader 1 of {1, 2}, committed = lastIndex = 1 (:1363); the
    heartbeat response from 2 (:1393) releases it: a MsgReadIndexResp to node 2
    = slot 1 at index 1."""
    be, S = Backend(eng), 2
    sc = _leader_after_hup(S)
    be.load(sc, initial_arrays(sc))
    res, ctx, index = be.read_index(key=0x637478, frm=1)
    assert (res, index) == (QUEUED, 1) and be.answers() == []
    out = _heartbeat_round(be, S, (1,), ctx=ctx)
    assert out["read_released"] == 1
    assert be.answers() == [(RESP, 1, ctx, 1, 0x637478)]
    assert be.queue()[0] == 0


def new_leader(last_index, followers):
    return {"name": "", "S": 3, "self": 0, "max_ents": 0,
            "log": {"runs": [[0, 0], [1, 1], [3, 2]], "committed": 1, "term_start": 3,
                    "first_index": 1, "last_index": last_index},
            "peers": [_peer(last_index, last_index + 1, 1)] + followers}


def test_read_only_for_new_leader(eng):
    """TestReadOnlyForNewLeader (raft_test.go:2341-2410): windex = 4 (:2378);
    no ReadState while nothing of the term is committed (:2381); after the
    first commit in the term the postponed read is answered at windex (:2401-
    2407), and a second read too (:2414-2420)."""
    be, S = Backend(eng), 3
    sc = new_leader(3, [_peer(0, 3, 0, probe_sent=True) for _ in range(2)])
    be.load(sc, initial_arrays(sc))
    res, _, _ = be.read_index(key=0xC1)
    assert res == POSTPONED and be.answers() == []
    out = _heartbeat_round(be, S, (1, 2))
    assert out["term_commit"] == 0 and be.answers() == []
    assert be.propose(1)["result"] == 1
    z = np.zeros(S, np.uint64)
    out = be.step(np.array([0, 1, 1], np.uint8), np.array([0, 4, 4], np.uint64), z, z)
    assert be.committed() == 4 and out["term_commit"] == 1
    assert be.answers() == [(TERM_COMMIT, NONE, 0, 4, 0)]
    tci = out["term_commit_index"]
    res, ctx, index = be.read_index(key=0xC1, at=tci)  # the postponed read, added again
    assert res == QUEUED and be.answers() == []
    out = _heartbeat_round(be, S, (1, 2), ctx=ctx)
    assert out["read_released"] == 1
    assert be.answers() == [(STATE, NONE, ctx, 4, 0xC1)]
    res, ctx2, index = be.read_index(key=0xC2)
    assert res == QUEUED and ctx2 == ctx + 1
    _heartbeat_round(be, S, (1, 2), ctx=ctx2)
    assert be.answers() == [(STATE, NONE, ctx2, 4, 0xC2)]


def test_postponed_read_commit_advances_twice(eng):
    """The round whose commit advances twice (leader_round_scenarios.
    postponed_read_commit_advances_twice; raft.go:1259-1262, :1813-1834): the
    postponed read is answered at term_commit_index 4, not at the committed
    index 5 the re-adding qe_read_index returns."""
    be, S = Backend(eng), 3
    sc = new_leader(5, [_peer(2, 6, 1, True) for _ in range(2)])
    be.load(sc, initial_arrays(sc))
    assert be.read_index(key=7)[0] == POSTPONED
    z = np.zeros(S, np.uint64)
    out = be.step(np.array([0, 1, 1], np.uint8), np.array([0, 4, 5], np.uint64), z, z)
    assert out["term_commit"] == 1 and be.committed() == 5
    assert be.answers() == [(TERM_COMMIT, NONE, 0, 4, 0)]
    res, ctx, index = be.read_index(key=7, frm=2, at=out["term_commit_index"])
    assert (res, index) == (QUEUED, 5)
    _heartbeat_round(be, S, (1, 2), ctx=ctx)
    assert be.answers() == [(RESP, 2, ctx, 4, 7)]


# ---- the random differential ----

def random_queues(rng, pb, cap_arg, keys):
    """Random queues of 0..cap pending requests (most past the word), random
    acks (dead slots hold garbage), heads near 1 and just below 2^32 (a
    pending queue never crosses context 0), random keys."""
    pb.track_reads(cap_arg, keys=keys)
    G, cap = pb.G, max(4, cap_arg)
    deep = rng.random(G) < 0.7
    cnt = np.where(deep, rng.integers(min(5, cap), cap + 1, G), rng.integers(0, 5, G))
    near = rng.integers((1 << 32) - 2 * cap - 2, (1 << 32) - 1, G, dtype=np.uint64)
    pb.read_head[:] = np.where(rng.random(G) < 0.5, rng.integers(1, 1000, G), near).astype(np.uint32)
    pb.read_count[:] = np.minimum(cnt, (1 << 32) - 1 - pb.read_head.astype(np.int64))
    pb.read_acks[:] = rng.integers(0, 1 << 62, G, dtype=np.uint64).astype(pb.read_acks.dtype)
    if pb.read_ovf is not None:
        pb.read_ovf[:] = rng.integers(0, 1 << 16, pb.read_ovf.size).astype(pb.read_ovf.dtype)
    if keys:
        pb.read_keys[:] = rng.integers(0, 1 << 62, pb.read_keys.size, dtype=np.uint64)


def random_ctx(rng, S, head, cnt):
    """Contexts of the heartbeat responses: mostly pending ones, some released,
    some never assigned, some none."""
    n = S * head.size
    h, c = np.tile(head, S).astype(np.int64), np.tile(cnt, S).astype(np.int64)
    pick = rng.integers(0, 6, n)
    ctx = np.where(pick == 0, 0, np.where(pick == 1, h - rng.integers(1, 4, n), np.where(
        pick == 2, h + c + rng.integers(0, 3, n), h + rng.integers(0, 1 << 20, n) % np.maximum(c, 1))))
    return (ctx & M32).astype(np.uint32)


def compare(eng, rs, recs, stats_dev, stats, where):
    count, got = rs.records()
    assert count == len(recs), (where, count, len(recs))
    want = rsm.columns(recs, rs.capacity)
    for k in rsm.FIELDS:
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{where} {k}")
    if stats_dev is not None:
        folded = eng.stats_reduce(stats_dev).cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(folded, np.array(stats, np.uint64), err_msg=f"{where} stats")


CASES = [(1, 3, 0, True), (63, 5, 255, True), (65, 10, 16, False), (4097, 3, 5, True),
         (2 * 4096 + 209, 5, 16, True), (65, 3, 255, False), (4097, 10, 0, False)]


@pytest.mark.parametrize("G,S,cap_arg,keys", CASES)
def test_read_states_match_model(eng, G, S, cap_arg, keys):
    """read_index -> read_note -> progress_step (MsgHeartbeatResp, random
    contexts) -> read_states, the whole list, count, statistics and both book
    rows against the model every round.  Some groups have one voter (IsSingleton:
    immediate answers), some have nothing of their term committed (POSTPONED,
    then TERM_COMMIT)."""
    rng = np.random.default_rng(7300 + G + 17 * S + cap_arg)
    cap, goff = max(4, cap_arg), 1_000_003
    pb = random_state(rng, G, S, 8, 3, ("inc",), EXTRAS, max_ents=1)
    pb.tracked[:] = (1 << S) - 1
    pb.inc[:] = np.where(rng.random(G) < 0.15, 1 << rng.integers(0, S, G), (1 << S) - 1)
    pb.self_slot[:] = rng.integers(0, S + 1, G)  # (S: no slot of its own)
    random_queues(rng, pb, cap_arg, keys)
    ps = to_device(eng, pb, ("inc",), EXTRAS + ("reads",))
    ps.group_offset = goff
    book, mb = eng.ReadBook(ps), rsm.Book(G, cap_arg)
    mb.req_index[:] = rng.integers(0, 1 << 62, mb.req_index.size, dtype=np.uint64)
    mb.req_from[:] = np.where(rng.random(mb.req_from.size) < 0.5, NONE,
                              rng.integers(0, S + 2, mb.req_from.size))
    book.load_host(req_index=mb.req_index, req_from=mb.req_from)
    rs = eng.ReadStates(ps, G * (cap + 2), key=keys or G != 65)
    seen = set()
    for rnd in range(3):
        h = ps.host()
        req = (rng.random(G) < 0.8).astype(np.uint8)
        key = rng.integers(0, 1 << 62, G, dtype=np.uint64)
        if keys:  # some requests resent: pending already
            cnt = h["read_count"].astype(np.int64)
            at = (h["read_head"].astype(np.int64) + rng.integers(0, 1 << 20, G) % np.maximum(cnt, 1)) % cap
            dup = (rng.random(G) < 0.3) & (cnt > 0)
            key = np.where(dup, h["read_keys"].reshape(G, cap)[np.arange(G), at], key)
        frm = np.where(rng.random(G) < 0.4, NONE, rng.integers(0, S + 2, G)).astype(np.uint8)
        kt, ft = (i64(key) if keys else None), u8(frm)
        res, ctx, index = eng.read_index(ps, u8(req), False, key=kt)
        eng.read_note(ps, book, res, ctx, index, ft)
        r_h, c_h = res.cpu().numpy(), ctx.cpu().numpy().view(np.uint32)
        i_h = index.cpu().numpy().view(np.uint64)
        rsm.read_note(mb, r_h, c_h, i_h, frm)
        seen |= set(int(x) for x in np.unique(r_h))
        h = ps.host()
        mtype, mindex, mhint, mlogterm = random_msgs(rng, pb)
        mtype[rng.random(mtype.size) < 0.6] = 3
        msgs = load_msgs(eng, ps, mtype, mindex, mhint, mlogterm)
        msgs.set_read_ctx(ps, random_ctx(rng, S, h["read_head"], h["read_count"]))
        eng.progress_step(ps, msgs)
        stats = eng.stats_buffer(DEV)
        eng.read_states(ps, book, rs, msgs=msgs, ri=(res, ctx, index, ft, kt), stats=stats)
        h = ps.host()
        rel = msgs.read_released.cpu().numpy()
        tc = msgs.term_commit.cpu().numpy()
        recs, want_stats = rsm.read_states(
            G, S, cap_arg, h["read_head"], mb, h["self_slot"], h["read_keys"], goff,
            read_released=rel, term_commit=tc,
            term_commit_index=msgs.term_commit_index.cpu().numpy().view(np.uint64),
            ri_result=r_h, ri_index=i_h, ri_from=frm, ri_key=key if keys else None)
        compare(eng, rs, recs, stats, want_stats, f"round {rnd}")
        bh = book.host()
        np.testing.assert_array_equal(bh["req_index"], mb.req_index, err_msg="req_index")
        np.testing.assert_array_equal(bh["req_from"], mb.req_from, err_msg="req_from")
        seen |= {10 + r["kind"] for r in recs} | {100 + min(int(rel.max()), 2)}
    if G >= 63:  # every result and every kind of record came up
        assert {_lib.QE_RI_RESPOND, _lib.QE_RI_QUEUED, 10 + STATE, 10 + RESP, 102} <= seen, seen
        assert not keys or _lib.QE_RI_DUPLICATE in seen
    if G >= 4097:
        assert _lib.QE_RI_POSTPONED in seen and 10 + TERM_COMMIT in seen, seen


# ---- extremes and capacity ----

def rows_state(eng, rng, G, S, cap_arg, keys=True):
    """A state of which qe_read_states reads read_head, self_slot and
    read_keys, and a book, both random; -> (ps, book, the model's book, the
    host rows)."""
    extras = ("self_slot", "reads") + (("read_keys",) if keys else ())
    ps = eng.ProgressState(G, S, 4, 2, DEV, extras=extras, read_cap=cap_arg)
    cap = max(4, cap_arg)
    head = rng.integers(300, 1 << 32, G, dtype=np.uint64).astype(np.uint32)
    me = rng.integers(0, S + 1, G).astype(np.uint8)
    rk = rng.integers(0, 1 << 62, G * cap, dtype=np.uint64) if keys else None
    ps.load_host(read_head=head, self_slot=me, read_keys=rk)
    book, mb = eng.ReadBook(ps), rsm.Book(G, cap_arg)
    mb.req_index[:] = rng.integers(0, 1 << 62, mb.req_index.size, dtype=np.uint64)
    mb.req_from[:] = rng.integers(0, S + 2, mb.req_from.size)
    book.load_host(req_index=mb.req_index, req_from=mb.req_from)
    return ps, book, mb, SimpleNamespace(head=head, me=me, keys=rk)


def sentinel(eng, ps, rows, capacity):
    """A ReadStates of `rows` records filled with a sentinel, of which the call
    may write `capacity`."""
    rs = eng.ReadStates(ps, rows)
    for k in rs.ARRAYS:
        getattr(rs, k).fill_(0x5A)
    rs.capacity = capacity
    return rs


def untouched(rs, frm, rows):
    for k, a in rs.host().items():
        if k != "count":
            assert (a[frm:rows] == 0x5A).all(), k


def test_nothing_to_list(eng):
    """Every row NULL, or every row zero: count 0, nothing written."""
    rng = np.random.default_rng(7401)
    G = 4096 + 70
    ps, book, mb, h = rows_state(eng, rng, G, 3, 16)
    rs = sentinel(eng, ps, 64, 64)
    eng.read_states(ps, None, rs)
    assert int(rs.count.item()) == 0
    untouched(rs, 0, 64)
    rs.count.fill_(77)
    z8 = torch.zeros(G, dtype=torch.uint8, device=DEV)
    z64 = torch.zeros(G, dtype=torch.int64, device=DEV)
    stats = eng.stats_buffer(DEV)
    eng.read_states(ps, book, rs, SimpleNamespace(read_released=z8, term_commit=z8,
                                                  term_commit_index=z64),
                    ri=(z8, None, z64), stats=stats)
    assert int(rs.count.item()) == 0
    untouched(rs, 0, 64)
    assert not eng.stats_reduce(stats).cpu().numpy().any()


@pytest.mark.parametrize("empty", [True, False])
def test_empty_batch_and_absent_rows_through_the_c_call(eng, empty):
    """num_groups == 0 (rows given), or every row of `in` NULL: QE_OK with
    *count = 0, and then the book, the queue, self_slot, read_keys, scratch (an
    empty batch), `key` and, with capacity 0, every record array may be NULL."""
    import ctypes as C

    count = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(64, dtype=torch.int64, device=DEV)
    V = C.c_void_p(scratch.data_ptr())
    p = _lib.QeProgress(num_groups=0 if empty else 4, num_slots=3, inflight_cap=4,
                        stride=0 if empty else 4, log_runs=2)
    i = _lib.QeReadStatesIn()
    if empty:
        i.term_commit = i.term_commit_index = i.ri_result = i.ri_index = V
    o = _lib.QeReadStatesOut(capacity=0, count=C.c_void_p(count.data_ptr()))
    rc = _lib.lib().qe_read_states(C.byref(p), None, C.byref(i), C.byref(o),
                                   None if empty else V, None, None)
    assert rc == _lib.QE_OK
    torch.cuda.synchronize()
    assert int(count.item()) == 0


def extreme_rows(rng, G):
    """One group releasing 255 requests beside groups releasing none, a few
    small runs around it, and one tile (the second) in which every group has a
    TERM_COMMIT and an immediate answer."""
    rel = np.zeros(G, np.uint8)
    rel[70], rel[5], rel[69], rel[71], rel[G - 1] = 255, 3, 1, 2, 4
    tc = np.zeros(G, np.uint8)
    res = np.zeros(G, np.uint8)
    tc[64:128], res[64:128] = 1, _lib.QE_RI_RESPOND
    tc[3], res[G - 2] = 1, _lib.QE_RI_RESPOND
    res[7] = _lib.QE_RI_QUEUED  # (no answer)
    tci = rng.integers(1, 1 << 40, G, dtype=np.uint64)
    ri_index = rng.integers(1, 1 << 40, G, dtype=np.uint64)
    ri_from = rng.integers(0, 6, G).astype(np.uint8)
    ri_key = rng.integers(0, 1 << 62, G, dtype=np.uint64)
    return rel, tc, tci, res, ri_index, ri_from, ri_key


def run_extreme(eng, rng, G, S, capacity, rows, stats=True):
    ps, book, mb, h = rows_state(eng, rng, G, S, 255)
    rel, tc, tci, res, ri_index, ri_from, ri_key = extreme_rows(rng, G)
    rs = sentinel(eng, ps, rows, capacity)
    st = eng.stats_buffer(DEV) if stats else None
    eng.read_states(ps, book, rs,
                    SimpleNamespace(read_released=u8(rel), term_commit=u8(tc),
                                    term_commit_index=i64(tci)),
                    ri=(u8(res), None, i64(ri_index), u8(ri_from), i64(ri_key)), stats=st)
    recs, want_stats = rsm.read_states(G, S, 255, h.head, mb, h.me, h.keys, 0, read_released=rel,
                                       term_commit=tc, term_commit_index=tci, ri_result=res,
                                       ri_index=ri_index, ri_from=ri_from, ri_key=ri_key)
    compare(eng, rs, recs, st, want_stats, f"capacity {capacity}")
    untouched(rs, min(capacity, len(recs)), rows)
    return recs


def test_one_group_with_255_records_and_a_full_tile(eng):
    rng = np.random.default_rng(7402)
    G = 3 * 64 + 9
    recs = run_extreme(eng, rng, G, 5, 600, 640)
    assert len(recs) == 255 + 3 + 1 + 2 + 4 + 2 * 64 + 2
    run = [r for r in recs if r["group"] == 70]
    assert len(run) == 257
    assert [r["kind"] for r in run[255:]] in ([TERM_COMMIT, STATE], [TERM_COMMIT, RESP])
    ctxs = [r["ctx"] for r in run[:255]]
    assert ctxs == [(ctxs[0] + j) & M32 for j in range(255)]  # oldest first


@pytest.mark.parametrize("capacity", [0, 1, 3, 4, 100, 272, 273, 394])
def test_capacity_cuts(eng, capacity):
    """capacity below count -- at 0, after the first record, inside a group's
    run, between two groups, in the middle of the 255-request run, at its end,
    between its TERM_COMMIT and its immediate answer and one short of
    everything: count stays full, the prefix
    is exact, and the sentinel past capacity and in the guard rows behind the
    arrays stays."""
    rng = np.random.default_rng(7402)
    recs = run_extreme(eng, rng, 3 * 64 + 9, 5, capacity, capacity + 64, stats=capacity % 2 == 0)
    assert len(recs) == 395 and capacity < len(recs)


def test_fill_blocks_walk(eng):
    """test_fill_blocks_walk of tests/test_gpu_outbox.py for qe_read_states,
    the one list whose tile holds runs of 0..257 records per group and loads
    the book after stores: a quiet batch of one chunk more than the capped fill
    grid has blocks, so that with statistics a block takes a second chunk.
    About 1% of the groups release 1..3 reads (some forwarded: a
    MsgReadIndexResp), a few have a TERM_COMMIT notice, a few an immediate
    answer; read_cap 4.  The list of the call with statistics against the list
    of the call without (a block per chunk, what the model tests pin), and the
    per-kind counters against the kinds in the list."""
    from tests.test_gpu_outbox import GOFF, DeviceRandom, same_list, walk_groups
    e, L = eng, _lib
    G, S, cap = walk_groups(), 2, 4
    rnd = DeviceRandom(G, 0x0E5D)
    t8, zero = torch.uint8, torch.zeros(G, dtype=torch.uint8, device=DEV)
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF,
                         extras=("self_slot", "reads", "read_keys"), read_cap=cap)
    ps.read_head.copy_(rnd.ints(300, 1 << 31, torch.int32))
    ps.self_slot.copy_(rnd.ints(0, S + 1, t8))
    ps.read_keys.copy_(torch.randint(0, 1 << 62, (G * cap,), generator=rnd.gen, device=DEV))
    book = e.ReadBook(ps)
    book.req_index.copy_(torch.randint(1, 1 << 40, (G * cap,), generator=rnd.gen, device=DEV))
    book.req_from.copy_(torch.randint(0, S + 2, (G * cap,), generator=rnd.gen, device=DEV).to(t8))
    rel = torch.where(rnd.hit(0.01), rnd.ints(1, 4, t8), zero)
    msgs = SimpleNamespace(read_released=rel, term_commit=rnd.hit(0.002).to(t8),
                           term_commit_index=rnd.ints(1, 1 << 40))
    res = torch.where(rnd.hit(0.003), torch.full_like(zero, L.QE_RI_RESPOND),
                      torch.where(rnd.hit(0.01), torch.full_like(zero, L.QE_RI_QUEUED), zero))
    ri = (res, None, rnd.ints(1, 1 << 40), rnd.ints(0, S + 2, t8), rnd.ints(0, 1 << 62))
    want = int((rel.sum() + msgs.term_commit.sum() + (res == L.QE_RI_RESPOND).sum()).item())
    lists = []
    for stats in (None, e.stats_buffer(DEV)):
        rs = e.ReadStates(ps, want + 5)
        e.read_states(ps, book, rs, msgs=msgs, ri=ri, stats=stats)
        lists.append(rs)
    n = same_list(lists[0], lists[1], (), 0)
    assert n == want
    folded = e.stats_reduce(stats)
    kind = lists[0].kind[:n]
    per_kind = {L.QE_STAT_READ_STATE: STATE, L.QE_STAT_READ_RESP: RESP,
                L.QE_STAT_READ_TERM_COMMIT: TERM_COMMIT}
    for stat, k in per_kind.items():
        assert int(folded[stat].item()) == int((kind == k).sum().item()) > 0, ("stat", stat)
    assert sum(int(folded[stat].item()) for stat in per_kind) == n  # the record count
    groups = int(((rel != 0) | (msgs.term_commit != 0) | (res == L.QE_RI_RESPOND)).sum().item())
    assert int(folded[0].item()) == groups  # QE_STAT_GROUPS: the groups with a record
