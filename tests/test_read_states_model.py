"""tests/read_states_model.py (the row-level restatement of qe_read_note /
qe_read_states, the checker of the GPU tests) held against an independent
raft/read_only.go kept as Python lists, the way the reference keeps it -- the
`Model` of tests/test_readonly_model.py with what readIndexStatus holds
besides the acks:

  readIndexQueue / pendingReadIndex -> per request [ctx, acks, key, index, from]
  addRequest (:56-63)   index = the commit index when the request arrived
  advance    (:81-112)  the released requests, oldest first
  responseToReadIndexReq (raft.go:1737-1751): req.From == None || == r.id ->
      ReadState{Index, RequestCtx}, else MsgReadIndexResp{To: req.From, Index}

The queue itself (acks, head, count, keys) is the oracle's, driven through
orc.read_index / orc.progress_step; the answers of the reference form must
equal the list record by record.  CPU only."""
import numpy as np
import pytest

from etcd_amd import _lib
from oracle import orc
from tests import read_states_model as rsm
from tests.test_gpu_progress import EXTRAS, random_msgs, random_state

M32 = 0xFFFFFFFF


class Model:
    """One group's readOnly, ReadOnlySafe, with the requests' index and origin."""

    def __init__(self, head):
        self.head = head
        self.q = []  # [ctx, acks, key, index, from] in arrival order

    def add(self, self_bit, key, index, frm, cap):
        for e in self.q:
            if e[2] == key:
                return _lib.QE_RI_DUPLICATE, e[0]
        if not self.q and self.head == 0:
            self.head = 1
        ctx = (self.head + len(self.q)) & M32
        if len(self.q) >= cap or ctx == 0:
            return _lib.QE_RI_FULL, None
        self.q.append([ctx, self_bit, key, index, frm])
        return _lib.QE_RI_QUEUED, ctx

    def ack(self, slot, ctx, voters):
        """recvAck + advance on a won vote -> the released requests."""
        if ctx == 0:
            return []
        for j, e in enumerate(self.q):
            if e[0] == ctx:
                e[1] |= 1 << slot
                if bin(e[1] & voters).count("1") >= bin(voters).count("1") // 2 + 1:
                    rel = self.q[:j + 1]
                    del self.q[:j + 1]
                    self.head = (self.head + j + 1) & M32
                    return rel
                return []
        return []


def respond(gid, frm, me, S, ctx, index, key):
    """responseToReadIndexReq, as a record."""
    local = frm >= S or frm == me  # (a slot >= S is None)
    return dict(group=gid, kind=rsm.RS_STATE if local else rsm.RS_RESP, to=0xFF if local else frm,
                ctx=ctx, index=index, key=key)


def origins(rng, pb):
    """req.From per group: None, the leader itself, a peer, or a slot past S."""
    G, S = pb.G, pb.S
    pick = rng.integers(0, 4, G)
    return np.where(pick == 0, 0xFF, np.where(pick == 1, pb.self_slot, np.where(
        pick == 2, rng.integers(0, S, G), rng.integers(S, 256, G)))).astype(np.uint8)


def setup(rng, G, S, cap):
    """Random queues of 0..cap pending requests, heads near 1 and near 2^32,
    with the book and the reference-form model holding the same requests."""
    pb = random_state(rng, G, S, 8, 3, (), EXTRAS, max_ents=1)
    full = (1 << S) - 1
    pb.tracked[:] = full
    pb.self_slot[:] = rng.integers(0, S, G)
    pb.term_start[:] = np.minimum(pb.term_start, pb.last_index)
    pb.committed[:] = pb.last_index
    pb.track_reads(0 if cap == 4 else cap, keys=True)
    pb.read_count[:] = np.where(rng.random(G) < 0.6, rng.integers(0, cap + 1, G),
                                rng.integers(0, min(cap, 4) + 1, G))
    near = rng.integers((1 << 32) - 2 * cap - 2, (1 << 32) - 1, G, dtype=np.uint64)
    pb.read_head[:] = np.where(rng.random(G) < 0.5, rng.integers(1, 1000, G), near).astype(np.uint32)
    # a pending queue never crosses context 0
    room = (1 << 32) - 1 - pb.read_head.astype(np.int64)
    pb.read_count[:] = np.minimum(pb.read_count, room)
    pb.read_acks[:] = 0
    if pb.read_ovf is not None:
        pb.read_ovf[:] = 0
    pb.read_keys[:] = rng.permutation(pb.read_keys.size).astype(np.uint64) * 7919 + 1
    book = rsm.Book(G, pb.read_cap)
    book.req_index[:] = rng.integers(0, 1 << 62, book.req_index.size, dtype=np.uint64)  # dead slots
    book.req_from[:] = rng.integers(0, 256, book.req_from.size)
    models = []
    keys = pb.read_keys.reshape(G, cap)
    for g in range(G):
        m = Model(int(pb.read_head[g]))
        for j in range(int(pb.read_count[g])):
            c = (m.head + j) & M32
            e = g * cap + c % cap
            book.req_index[e] = rng.integers(1, 1 << 40)
            book.req_from[e] = rng.choice([0xFF, int(pb.self_slot[g]), int(rng.integers(0, S)), S])
            m.q.append([c, 0, int(keys[g, c % cap]), int(book.req_index[e]), int(book.req_from[e])])
        models.append(m)
    return pb, book, models


def run(rng, G, S, cap, rounds, wrong_note=False):
    """-> the kinds of records seen; raises AssertionError where the list and
    the reference form part."""
    pb, book, models = setup(rng, G, S, cap)
    full, seen, multi = (1 << S) - 1, set(), 0
    for rnd in range(rounds):
        want = [[] for _ in range(G)]
        if rnd % 3 == 0:  # MsgReadIndex: fresh keys, keys already pending, every origin
            req = (rng.random(G) < 0.8).astype(np.uint8)
            key = rng.integers(1 << 40, 1 << 62, G, dtype=np.uint64)
            for g in range(G):
                if models[g].q and rng.random() < 0.3:
                    key[g] = models[g].q[int(rng.integers(0, len(models[g].q)))][2]
            frm = origins(rng, pb)
            committed = pb.committed.copy()
            res, ctx, index = orc.read_index(pb, req, False, key=key)
            for g in range(G):
                if not req[g]:
                    continue
                r, _ = models[g].add(1 << int(pb.self_slot[g]), int(key[g]), int(committed[g]),
                                     int(frm[g]), cap)
                assert res[g] == r, (rnd, g, res[g], r)
            noted = index + np.uint64(1) if wrong_note else index
            rsm.read_note(book, res, ctx, noted, frm)
            recs, stats = rsm.read_states(G, S, pb.read_cap, pb.read_head, book, pb.self_slot,
                                          pb.read_keys, 7, ri_result=res, ri_index=index,
                                          ri_from=frm, ri_key=key)
            assert not (res == _lib.QE_RI_RESPOND).any()  # ReadOnlySafe, no singleton
        elif rnd % 3 == 1 and rnd % 6 == 4:  # ReadOnlyLeaseBased: the immediate answers
            req = (rng.random(G) < 0.5).astype(np.uint8)
            key = rng.integers(1 << 40, 1 << 62, G, dtype=np.uint64)
            frm = origins(rng, pb)
            res, ctx, index = orc.read_index(pb, req, True, key=key)
            for g in np.nonzero(req)[0]:
                assert res[g] == _lib.QE_RI_RESPOND
                want[g].append(respond(7 + int(g), int(frm[g]), int(pb.self_slot[g]), S, 0,
                                       int(pb.committed[g]), int(key[g])))
            rsm.read_note(book, res, ctx, index, frm)  # (nothing queued: writes nothing)
            recs, stats = rsm.read_states(G, S, pb.read_cap, pb.read_head, book, pb.self_slot,
                                          pb.read_keys, 7, ri_result=res, ri_index=index,
                                          ri_from=frm, ri_key=key)
        else:  # one round of MsgHeartbeatResp: contexts anywhere in the queue
            mtype, mindex, mhint, mlogterm = random_msgs(rng, pb)
            mtype[:] = np.where(rng.random(mtype.size) < 0.7, 3, 0).astype(mtype.dtype)
            cx = np.zeros(S * G, np.uint32)
            for g in range(G):
                h, n = models[g].head, len(models[g].q)
                for s in range(S):
                    pick = rng.integers(0, 5)
                    cx[s * G + g] = (0 if pick == 0 else
                                     (h - int(rng.integers(1, 4))) & M32 if pick == 1 else
                                     (h + n + int(rng.integers(0, 3))) & M32 if pick == 2 else
                                     (h + int(rng.integers(0, max(n, 1)))) & M32)
            o = orc.progress_step(pb, mtype, mindex, mhint, mlogterm, read_ctx=cx)
            for g in range(G):
                m, times = models[g], 0
                for s in range(S):
                    if mtype[s * G + g] == 3:
                        rel = m.ack(s, int(cx[s * G + g]), full)
                        times += 1 if rel else 0
                        for c, _, key, index, frm in rel:
                            want[g].append(respond(7 + g, frm, int(pb.self_slot[g]), S, c, index,
                                                   key))
                multi += times > 1
                assert int(o.read_released[g]) == len(want[g]), (rnd, g)
                if o.term_commit[g]:
                    want[g].append(dict(group=7 + g, kind=rsm.RS_TERM_COMMIT, to=0xFF, ctx=0,
                                        index=int(o.term_commit_index[g]), key=0))
            recs, stats = rsm.read_states(G, S, pb.read_cap, pb.read_head, book, pb.self_slot,
                                          pb.read_keys, 7, read_released=o.read_released,
                                          term_commit=o.term_commit,
                                          term_commit_index=o.term_commit_index)
        flat = [r for w in want for r in w]
        assert recs == flat, (rnd, [(a, b) for a, b in zip(recs, flat) if a != b][:3])
        assert stats[rsm.STAT_GROUPS] == sum(1 for w in want if w)
        for kind, at in rsm.BY_KIND.items():
            assert stats[at] == sum(r["kind"] == kind for r in flat)
        seen |= {r["kind"] for r in flat}
        seen |= {100 + min(len(w), 9) for w in want}
        for g in range(G):  # the queue is the reference form's
            assert int(pb.read_head[g]) == models[g].head or not models[g].q, (rnd, g)
            assert int(pb.read_count[g]) == len(models[g].q), (rnd, g)
    return seen, multi


@pytest.mark.parametrize("S", [3, 5, 10])
@pytest.mark.parametrize("cap", [4, 5, 16, 255])
def test_list_equals_reference_form(S, cap):
    rng = np.random.default_rng(6200 + 31 * S + cap)
    seen, multi = run(rng, 97, S, cap, 12)
    assert {rsm.RS_STATE, rsm.RS_RESP} <= seen
    assert any(v >= 102 for v in seen), sorted(seen)  # several requests released in one round
    if cap > 4 and S == 3:  # (a quorum of two: two contexts can win in one round)
        assert multi  # ... by more than one advance of the same round


def test_a_book_entry_noted_at_the_wrong_index_fails():
    """The control: with qe_read_note fed index + 1 the list no longer equals
    the reference form."""
    with pytest.raises(AssertionError):
        run(np.random.default_rng(6299), 97, 5, 16, 12, wrong_note=True)
    run(np.random.default_rng(6299), 97, 5, 16, 12)  # the same run, noted right
