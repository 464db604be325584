"""The closed loop of client requests, on the device: 211 three-node clusters
in the layout of tests/test_gpu_read_states_loop.py (node i of cluster c is
group 3c + i, sits in slot i and has self_slot = i).  Reads, proposals and one
leadership transfer per cluster are issued at random nodes, followers included,
as local calls (from = None, term 0).  One pass:

  every node:  requests            (followers: FWD records; leaders: the rows)
  leaders:     propose -> outbox -> [inbox, follower_step, replies, inbox, progress_step]
               read_index -> read_note -> progress_step (the transfer rows)
               heartbeat -> outbox -> [the same exchange] -> read_states

The transport is done here: a FWD record goes to (cluster, `to`) with `from`
kept and arrives in the next pass's list behind that pass's deferred records;
a QE_RS_RESP goes to the follower as a READ_INDEX_RESP record and ends there
as a READ_STATE record.  Some heartbeats and responses are dropped.  Every pass
is also held against tests/requests_model.py.

The transfer runs on the device too: requests -> progress_step -> replies
(MsgTimeoutNow) -> inbox -> vote_step (the transferee campaigns) -> replies
(MsgVote) -> inbox -> vote_step (the others step down and grant) -> replies ->
inbox -> vote_step (won) -> become_leader -> outbox -> the exchange above.
Requests in flight to the old leader then arrive at a follower and are
forwarded once more, with `from` kept."""
import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import requests_model as qm
from tests.test_gpu_progress import DEV
from tests.test_gpu_requests import arrays, host, model_state

pytestmark = pytest.mark.gpu
N, C, CAP = 3, 211, 8
G = N * C
LEADER, REPLICATE, RECENT_ACTIVE = 2, 1, 8
RECORD = ("group", "type", "term", "index", "log_term", "commit", "hint", "ctx", "flags")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


class Loop:
    def __init__(self, e, seed):
        self.e, self.rng = e, np.random.default_rng(seed)
        rng = self.rng
        self.lead = np.repeat(np.arange(C) % N, N).astype(np.uint8)    # [G] the cluster's leader slot
        ps = self.ps = e.ProgressState(G, N, 8, 4, DEV, masks=("inc",), read_cap=CAP, extras=(
            "tracked", "self_slot", "reads", "read_keys", "lead_transferee"))
        st = ps.stride
        last = np.repeat(rng.integers(3, 40, C), N).astype(np.uint64)  # every log: 1..last at term 1
        self.first_last = last[::N].astype(np.int64)
        rows = np.zeros((4, st), np.uint64)
        rows[1, :G] = 1
        per = lambda a: np.pad(np.tile(a, (N, 1)), ((0, 0), (0, st - G)))  # noqa: E731
        ps.load_host(match=per(last), next=per(last + 1), committed=last, last_index=last,
                     term_start=np.ones(G, np.uint64), first_index=np.ones(G, np.uint64),
                     run_first=rows, run_term=rows, run_count=np.full(G, 2, np.uint8),
                     flags=per(np.full(G, REPLICATE | RECENT_ACTIVE, np.uint8)).reshape(-1),
                     tracked=np.full(G, 7, np.uint8), inc=np.full(G, 7, np.uint8),
                     self_slot=(np.arange(G) % N).astype(np.uint8))
        self.fol, self.voter = e.Follower(ps), e.Voter(ps)
        self.term = 1
        self.roles(self.lead)
        self.fol.load_host(term=np.ones(G, np.uint64), lead=self.lead,
                           state=np.where(self.is_leader, LEADER, 0).astype(np.uint8))
        self.book, self.rs = e.ReadBook(ps), e.ReadStates(ps, G * CAP)
        self.ob, self.rp = e.Outbox(ps, G * N, 1), e.Replies(ps, G)
        self.ib, self.rq = e.Inbox(ps, G * N, 1), e.Requests(ps, 16 * G)
        self.lm, self.fo = e.LeaderMsgs(ps, 1), e.FollowerOut(ps)
        self.sm, self.vm = e.SnapMsgs(ps), e.VoteMsgs(ps)
        self.queue, self.next_key = [], 1000
        self.reads, self.props = {}, {}        # key -> what the host knows of the request
        self.accepted = np.zeros(C, np.int64)  # entries the leaders appended for proposals
        self.timeout_now = {}                  # cluster -> the slot its leader sent MsgTimeoutNow to
        self.tnow = []                         # the MsgTimeoutNow records, in flight
        self.seen, self.dropped, self.reforwarded = set(), 0, 0

    def roles(self, lead):
        """What the host knows of who leads (the transport's and the clients' view)."""
        self.lead = lead
        self.is_leader = (np.arange(G) % N) == lead
        self.leader_t = torch.from_numpy(self.is_leader).to(DEV)

    def committed(self):
        return host(self.ps.committed)

    # ---- the transport of the replication messages (test_gpu_read_states_loop.py) ----
    def carry(self, count, recs, p_drop):
        assert count == len(recs["group"])  # (nothing cut by capacity)
        keep = self.rng.random(count) >= p_drop
        self.dropped += int(count - keep.sum())
        g = recs["group"].astype(np.int64)
        a = {k: recs[k][keep] for k in RECORD if recs.get(k) is not None}
        a["group"] = (g - g % N + recs["to"])[keep].astype(np.uint64)
        a["from"] = (g % N)[keep].astype(np.uint8)
        for k in ("ent_len", "ent_term"):
            a[k] = recs[k][:, keep] if recs.get(k) is not None else np.zeros((1, int(keep.sum())),
                                                                            np.uint64)
        a["ent_len"] = a["ent_len"].astype(np.uint32)
        self.ib.load_host(**a)
        return self.ib

    def exchange(self, p_drop):
        """What the leaders sent (self.ob), to the followers and back."""
        e, ps, fol = self.e, self.ps, self.fol
        ib = self.carry(*self.ob.records(), p_drop)
        pm = e.PeerMsgs(ps, outputs=False)
        e.inbox(ps, fol, ib, self.lm, self.sm, self.vm, pm)
        assert not int(ib.deferred_count.item())  # one message per follower and exchange
        e.follower_step(ps, fol, self.lm, self.fo)
        src = torch.where(self.lm.type != 0, ib.f_src, torch.zeros_like(ib.f_src)).to(torch.int64)
        f_ctx = torch.where(self.lm.type == _lib.QE_LMSG_HEARTBEAT, ib.ctx[src],
                            torch.zeros_like(ib.ctx[src]))
        e.replies(ps, fol.term, self.rp, follow=(self.lm, self.fo), f_ctx=f_ctx)
        ib = self.carry(*self.rp.records(), p_drop)
        pm = e.PeerMsgs(ps)
        pm.read_ctx = torch.zeros(N * ps.stride, dtype=torch.int32, device=DEV)
        e.inbox(ps, fol, ib, self.lm, self.sm, self.vm, pm)
        assert not int(ib.deferred_count.item())
        assert not self.lm.type.any() and not self.vm.type.any()  # responses only
        e.progress_step(ps, pm)
        assert not pm.snap.any()
        return pm

    # ---- the clients ----
    def key(self):
        self.next_key += 1
        return self.next_key

    def read(self, g):
        k = self.key()
        self.reads[k] = dict(node=g, c0=None, c1=None, done=False)
        return qm.rec(g, qm.READ_INDEX, key=k)

    def prop(self, g):
        k, ne = self.key(), int(self.rng.integers(1, 4))
        self.props[k] = dict(ne=ne, status=None)
        return qm.rec(g, qm.PROP, key=k, num_entries=ne)

    def clients(self, p_read, p_prop):
        rng, new = self.rng, []
        for g in rng.permutation(G):
            if rng.random() < p_read:
                new.append(self.read(int(g)))
            if rng.random() < p_prop:
                new.append(self.prop(int(g)))
        return new

    # ---- one pass ----
    def one_pass(self, new, p_drop):
        e, ps, fol, rq = self.e, self.ps, self.fol, self.rq
        recs, self.queue = self.queue + new, []
        pr, pm = e.Proposals(ps), e.PeerMsgs(ps)
        if recs:
            rq.load_host(**arrays(recs, 0))
        else:
            rq.n = 0
        e.requests(ps, fol, rq, pr, pm, self.vm)
        frows = dict(term=np.full(G, self.term), state=host(fol.state), lead=host(fol.lead),
                     self_slot=np.arange(G) % N)
        want = qm.route(model_state(G, N, 0, frows), recs)
        disp = rq.dispositions().tolist()
        assert disp == want.disposition
        assert not self.vm.type.any() and qm.BAD not in disp and qm.REF_PANIC not in disp
        self.seen.update(disp)
        count, out = rq.records()
        assert count == len(want.records) <= rq.capacity
        nxt = [recs[i] for i in rq.deferred]  # the next pass's list: the deferred records first
        for j in range(count):
            m, g, kind = recs[int(out["src"][j])], int(out["group"][j]), int(out["kind"][j])
            assert g == m["group"] and int(out["key"][j]) == m["key"]
            if kind == qm.QO_FWD:  # to the leader, `from` kept (the node's own slot for a local call)
                to, frm = int(out["to"][j]), int(out["from_"][j])
                assert to == self.lead[g] != g % N
                assert frm == (m["from"] if m["from"] < N else g % N)
                self.reforwarded += m["from"] < N and m["type"] != qm.TRANSFER_LEADER
                nxt.append(dict(m, group=g - g % N + to, term=int(out["term"][j]),
                                **{"from": frm}))
            elif kind == qm.QO_READ_STATE:  # the read ends where it was issued
                r = self.reads[m["key"]]
                assert not r["done"] and r["node"] == g
                assert r["c0"] <= int(out["index"][j]) == m["index"] <= r["c1"]
                r["done"] = True
            else:
                assert kind == qm.QO_PROP_DROPPED and self.props[m["key"]]["status"] is None
                self.props[m["key"]]["status"] = "dropped by requests"
        # ---- the leader side, in the order of rule 7 ----
        ne = host(pr.num_entries)
        if ne.any():
            before = ps.next.clone()
            e.propose(ps, pr)
            res, src = host(pr.result), host(rq.p_src)
            for g in np.flatnonzero(ne):
                p = self.props[recs[int(src[g])]["key"]]
                assert p["status"] is None and p["ne"] == ne[g] and self.is_leader[g]
                ok = res[g] == _lib.QE_PROP_OK
                assert ok or res[g] in (_lib.QE_PROP_DROPPED_NOT_MEMBER,
                                        _lib.QE_PROP_DROPPED_TRANSFER, _lib.QE_PROP_DROPPED_SIZE)
                p["status"] = "accepted" if ok else f"QE_PROP {res[g]}"
                self.accepted[g // N] += int(ne[g]) if ok else 0
            e.outbox(ps, fol.term, self.ob, sent=pr.sent, next_before=before)
            pm2 = self.exchange(0.0)
            assert not pm2.read_released.any()  # MsgAppResp releases nothing
        ri = e.read_index(ps, rq.ri_request, False, key=rq.ri_key)
        e.read_note(ps, self.book, *ri, rq.ri_from)
        res, src, c0 = host(ri[0]), host(rq.ri_src), self.committed()
        for g in np.flatnonzero(host(rq.ri_request)):
            m = recs[int(src[g])]
            assert self.is_leader[g] and res[g] in (_lib.QE_RI_QUEUED, _lib.QE_RI_FULL)
            if res[g] == _lib.QE_RI_QUEUED:
                self.reads[m["key"]]["c0"] = int(c0[g])
            else:  # the queue is full: the client tries again
                nxt.append(m)
        if pm.type.any():  # the transfers
            tl = host(pm.type).reshape(N, ps.stride)
            e.progress_step(ps, pm)
            e.replies(ps, fol.term, self.rp, timeout_now=pm.timeout_now)
            cnt, r = self.rp.records()
            assert cnt == int((tl == _lib.QE_MSG_TRANSFER_LEADER).sum())
            self.tnow.append(r)
            for j in range(cnt):
                g, to = int(r["group"][j]), int(r["to"][j])
                assert r["type"][j] == _lib.QE_IMSG_TIMEOUT_NOW and self.is_leader[g]
                assert tl[to, g] == _lib.QE_MSG_TRANSFER_LEADER and g // N not in self.timeout_now
                self.timeout_now[g // N] = to
        commit, hctx, sent = e.heartbeat(ps)
        sent = torch.where(self.leader_t, sent, torch.zeros_like(sent))  # MsgBeat at the leaders
        e.outbox(ps, fol.term, self.ob, hb_sent=sent, hb_commit=commit, hb_ctx=hctx)
        pm3 = self.exchange(p_drop)
        e.read_states(ps, self.book, self.rs, msgs=pm3, ri=ri + (rq.ri_from, rq.ri_key))
        count, r = self.rs.records()
        assert count <= self.rs.capacity
        now = self.committed()
        for j in range(count):
            g, kind, k = int(r["group"][j]), int(r["kind"][j]), int(r["key"][j])
            rd, idx = self.reads[k], int(r["index"][j])
            assert self.is_leader[g] and not rd["done"] and rd["c0"] <= idx <= int(now[g])
            if kind == _lib.QE_RS_STATE:  # issued at the leader itself
                assert rd["node"] == g
                rd["done"] = True
            else:  # MsgReadIndexResp to the follower the request came from
                assert kind == _lib.QE_RS_RESP and rd["c1"] is None
                to = int(r["to"][j])
                assert rd["node"] == g - g % N + to
                rd["c1"] = int(now[g])
                # (the response is not lost: a client's retry is not modelled)
                nxt.append(qm.rec(rd["node"], qm.READ_INDEX_RESP, g % N, self.term, idx, k))
        self.queue = nxt

    def deliver_votes(self, count, recs):
        """A list of election messages through inbox and vote_step, a pass per
        message of a group; -> the last pass's VoteOut.  A candidate that wins
        becomes leader before its next message."""
        e, ps, fol = self.e, self.ps, self.fol
        ib = self.carry(count, recs, 0.0)
        won = 0
        while True:
            e.inbox(ps, fol, ib, self.lm, self.sm, self.vm, e.PeerMsgs(ps, outputs=False))
            assert not self.lm.type.any() and not self.sm.type.any()
            vo = e.vote_step(ps, fol, self.voter, self.vm)
            assert not (host(vo.result) >= _lib.QE_VR_REFUSED).any()
            if vo.elected.any():
                won += int(vo.elected.sum())
                ld = e.Leader(ps, elected=vo.elected, bcast=True)
                ld.term.copy_(fol.term)
                e.become_leader(ps, ld)
                assert (host(ld.result)[host(vo.elected) != 0] == _lib.QE_BL_LEADER).all()
                e.outbox(ps, fol.term, self.ob, sent=ld.sent, next_before=ps.next)
            if not int(ib.deferred_count.item()):
                return vo, won
            ib = ib.gather_deferred()

    def elect_transferees(self):
        """The election the MsgTimeoutNow records in flight start."""
        e, ps, fol = self.e, self.ps, self.fol
        assert sorted(self.timeout_now) == list(range(C))
        assert not ps.read_count.any()  # (becomeFollower drops pending reads: there are none)
        lt, old = host(ps.lead_transferee), self.lead.copy()
        for c, to in self.timeout_now.items():
            assert lt[N * c + int(old[N * c])] == to != old[N * c]
        recs = {k: np.concatenate([r[k] for r in self.tnow]) for k in self.tnow[0]
                if self.tnow[0][k] is not None}
        vo, won = self.deliver_votes(C, recs)  # the transferees campaign
        res = host(vo.result)[host(self.vm.type) != 0]
        assert len(res) == C and (res == _lib.QE_VR_CAMPAIGN_VOTE).all() and not won
        e.replies(ps, fol.term, self.rp, vote=(self.vm, vo))
        cnt, r = self.rp.records()
        assert cnt == 2 * C and (r["type"] == _lib.QE_IMSG_VOTE).all()
        assert (r["flags"] & _lib.QE_VMF_FORCE).all()  # the transfer context
        vo, won = self.deliver_votes(cnt, r)  # the others step down and grant
        res = host(vo.result)[host(self.vm.type) != 0]
        assert len(res) == 2 * C and (res == _lib.QE_VR_GRANT).all() and not won
        e.replies(ps, fol.term, self.rp, vote=(self.vm, vo))
        cnt, r = self.rp.records()
        assert cnt == 2 * C and (r["type"] == _lib.QE_IMSG_VOTE_RESP).all()
        vo, won = self.deliver_votes(cnt, r)  # the first grant wins; the second meets a leader
        assert won == C
        self.term += 1
        assert (host(fol.term) == self.term).all()
        state = host(fol.state)
        new = np.repeat([self.timeout_now[c] for c in range(C)], N).astype(np.uint8)
        self.roles(new)
        assert ((state == LEADER) == self.is_leader).all() and not state[~self.is_leader].any()
        self.exchange(0.0)  # the empty entry of the new term, replicated and committed
        np.testing.assert_array_equal(host(fol.lead), new)  # everyone follows the transferee
        assert (host(ps.lead_transferee) == 0xFF).all()
        return old


def test_requests_at_any_node_reach_the_leader_and_their_answers_come_back(eng):
    lp = Loop(eng, 8102)
    rng = lp.rng
    for rnd in range(8):
        lp.one_pass(lp.clients(0.25, 0.2), 0.3)
    while lp.queue or lp.ps.read_count.any():  # the network heals
        lp.one_pass([], 0.0)
    assert all(r["done"] for r in lp.reads.values())
    # ---- one transfer per cluster, issued at a random node, a proposal right behind it ----
    new = []
    for c in range(C):
        at, to = N * c + int(rng.integers(0, N)), (c % N + int(rng.integers(1, N))) % N
        new += [qm.rec(at, qm.TRANSFER_LEADER, to), lp.prop(at)]
    lp.one_pass(new, 0.0)
    at_leader = len(lp.timeout_now)
    assert 0 < at_leader < C  # the others were forwarded: they arrive now
    # reads at the followers, in flight to the old leader during the election
    inflight = [lp.read(g) for g in range(G) if not lp.is_leader[g]]
    lp.one_pass(inflight, 0.0)
    old = lp.elect_transferees()
    before = lp.reforwarded
    lp.one_pass(lp.clients(0.25, 0.2), 0.0)
    # the requests in flight arrived at the old leader, a follower now: forwarded on, `from` kept
    assert lp.reforwarded - before >= len(inflight) == 2 * C and (old != lp.lead).all()
    for rnd in range(4):
        lp.one_pass(lp.clients(0.25, 0.2), 0.3)
    while lp.queue or lp.ps.read_count.any():
        lp.one_pass([], 0.0)
    lp.one_pass([], 0.0)  # (a last heartbeat carries the commit index to the followers)
    # ---- every read answered once, where it was issued; every proposal accounted for ----
    assert all(r["done"] for r in lp.reads.values()) and len(lp.reads) > 4 * C
    status = [p["status"] for p in lp.props.values()]
    assert None not in status and len(status) > 4 * C
    assert {"accepted", f"QE_PROP {_lib.QE_PROP_DROPPED_TRANSFER}"} <= set(status)
    last, commit = host(lp.ps.last_index).astype(np.int64), lp.committed().astype(np.int64)
    want = np.repeat(lp.first_last + lp.accepted + 1, N)  # (+ the new term's empty entry)
    np.testing.assert_array_equal(last, want)   # on all three logs ...
    np.testing.assert_array_equal(commit, want)  # ... and committed
    assert {qm.ROUTED, qm.DEFERRED, qm.FORWARDED, qm.READ_STATE} <= lp.seen
    assert lp.dropped > 0
