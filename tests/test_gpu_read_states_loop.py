"""The closed loop of a linearizable read, on the device: a few hundred 3-node
clusters (node i of cluster c is group 3c + i, sits in slot i and has
self_slot = i; the leader is node c % 3) driven through the existing calls

  leaders:    read_index -> read_note            (requests, some from followers)
              heartbeat -> outbox (ctx)           |  propose -> outbox (MsgApp)
  followers:  inbox -> follower_step -> replies (ctx)
  leaders:    inbox -> progress_step -> read_states

with the transport between outbox / replies and inbox done here (the mapping
of (sender group, `to`) to (receiver group, `from`) is the transport's, qe_inbox)
and some heartbeats and heartbeat responses dropped.  Rounds of proposals (no
drops: the followers stay in step) move the commit index between the reads.
Every request queued is answered exactly once, by the kind of record its
origin asks for (a ReadState for the leader's own and local requests, a
MsgReadIndexResp to the follower that sent it), with its key, at an index >=
the leader's commit index when it was queued and <= the commit index at its
release: the index readOnly.addRequest took (raft/read_only.go:56-63)."""
import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests.test_gpu_progress import DEV

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
        self.is_leader = (np.arange(G) % N) == self.lead
        ps = self.ps = e.ProgressState(G, N, 8, 2, DEV, extras=("tracked", "self_slot", "reads",
                                                                "read_keys"), read_cap=CAP)
        st = ps.stride
        last = np.repeat(rng.integers(3, 40, C), N).astype(np.uint64)  # every log: 1..last at term 1
        rows = np.zeros((2, st), np.uint64)
        rows[1, :G] = 1
        per = lambda a: np.pad(np.tile(a, (N, 1)), ((0, 0), (0, st - G)))  # noqa: E731
        ps.load_host(match=per(last), next=per(last + 1), committed=last, last_index=last,
                     term_start=np.ones(G, np.uint64), first_index=np.ones(G, np.uint64),
                     run_first=rows, run_term=rows, run_count=np.full(G, 2, np.uint8),
                     flags=per(np.full(G, REPLICATE | RECENT_ACTIVE, np.uint8)).reshape(-1),
                     tracked=np.full(G, 7, np.uint8), self_slot=(np.arange(G) % N).astype(np.uint8))
        fol = self.fol = e.Follower(ps)
        fol.load_host(term=np.ones(G, np.uint64), lead=self.lead,
                      state=np.where(self.is_leader, LEADER, 0).astype(np.uint8))
        self.book, self.rs = e.ReadBook(ps), e.ReadStates(ps, G * CAP)
        self.ob, self.rp = e.Outbox(ps, G * N, 1), e.Replies(ps, G)
        self.ib = e.Inbox(ps, G * N, 1)
        self.lm, self.fo = e.LeaderMsgs(ps, 1), e.FollowerOut(ps)
        self.sm, self.vm = e.SnapMsgs(ps), e.VoteMsgs(ps)
        self.leader_t = torch.from_numpy(self.is_leader).to(DEV)
        self.pending, self.answered, self.key = {}, 0, 1000
        self.kinds, self.dropped, self.full, self.spanned = set(), 0, 0, 0

    def committed(self):
        return self.ps.committed.cpu().numpy().view(np.uint64)

    # ---- the transport ----
    def carry(self, count, recs, p_drop):
        """A list of sent records (`group` the sender, `to` a slot) -> the Inbox:
        `group` the receiver, `from` the sender's slot; some are lost."""
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

    # ---- one exchange: what the leaders sent, to the followers and back ----
    def exchange(self, p_drop):
        e, ps, fol = self.e, self.ps, self.fol
        ib = self.carry(*self.ob.records(), p_drop)
        pm = e.PeerMsgs(ps, outputs=False)
        e.inbox(ps, fol, ib, self.lm, self.sm, self.vm, pm)
        assert not int(ib.deferred_count.item())  # one message per follower and round
        e.follower_step(ps, fol, self.lm, self.fo)
        # the context a heartbeat carried goes back with its response
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

    def propose_round(self):
        e, ps = self.e, self.ps
        pr = e.Proposals(ps)
        ne = np.where(self.is_leader & (self.rng.random(G) < 0.6), self.rng.integers(1, 4, G), 0)
        pr.num_entries.copy_(torch.from_numpy(ne.astype(np.int32)).to(DEV))
        before = ps.next.clone()
        e.propose(ps, pr)
        assert (pr.result.cpu().numpy()[ne > 0] == _lib.QE_PROP_OK).all()
        e.outbox(ps, self.fol.term, self.ob, sent=pr.sent, next_before=before)
        pm = self.exchange(0.0)
        # (the empty MsgApps of the bcastAppend after a commit, pm.sent, are lost here:
        # they carry the commit index alone, which the next heartbeat carries too)
        self.answers(pm, None)
        assert not self.rs.count.item()  # MsgAppResp releases nothing

    def read_round(self, p_req, p_drop):
        e, ps, rng = self.e, self.ps, self.rng
        req = self.is_leader & (rng.random(G) < p_req)
        frm = np.where(rng.random(G) < 0.5, 0xFF, rng.integers(0, N, G)).astype(np.uint8)
        key = (self.key + np.arange(G)).astype(np.uint64)
        self.key += G
        c0 = self.committed()
        ft = torch.from_numpy(frm).to(DEV)
        kt = torch.from_numpy(key.view(np.int64)).to(DEV)
        ri = e.read_index(ps, torch.from_numpy(req.astype(np.uint8)).to(DEV), False, key=kt)
        e.read_note(ps, self.book, *ri, ft)
        res, ctx = ri[0].cpu().numpy(), ri[1].cpu().numpy().view(np.uint32)
        assert set(np.unique(res[req])) <= {_lib.QE_RI_QUEUED, _lib.QE_RI_FULL}
        for g in np.flatnonzero(res == _lib.QE_RI_QUEUED):
            assert (int(g), int(ctx[g])) not in self.pending
            self.pending[int(g), int(ctx[g])] = (int(key[g]), int(frm[g]), int(c0[g]))
        self.full += int((res == _lib.QE_RI_FULL).sum())
        commit, hctx, sent = e.heartbeat(ps)
        sent = torch.where(self.leader_t, sent, torch.zeros_like(sent))  # MsgBeat at the leaders
        e.outbox(ps, self.fol.term, self.ob, hb_sent=sent, hb_commit=commit, hb_ctx=hctx)
        pm = self.exchange(p_drop)
        assert not pm.sent.any()  # every follower is in step: a response asks for nothing
        self.answers(pm, ri + (ft, kt))

    def answers(self, pm, ri):
        """The round's list against what the host knows of every request."""
        self.e.read_states(self.ps, self.book, self.rs, msgs=pm, ri=ri)
        count, r = self.rs.records()
        assert count <= self.rs.capacity
        now = self.committed()
        assert (np.diff(r["group"].astype(np.int64)) >= 0).all()  # by ascending group
        for n in range(count):
            g, kind = int(r["group"][n]), int(r["kind"][n])
            assert kind in (_lib.QE_RS_STATE, _lib.QE_RS_RESP), kind  # (ReadOnlySafe, term 1)
            key, frm, c0 = self.pending.pop((g, int(r["ctx"][n])))  # KeyError: answered twice
            assert int(r["key"][n]) == key
            assert c0 <= int(r["index"][n]) <= int(now[g]) and int(r["index"][n]) == c0
            self.spanned += c0 < int(now[g])
            local = frm >= N or frm == g % N
            assert kind == (_lib.QE_RS_STATE if local else _lib.QE_RS_RESP), (g, frm, kind)
            assert int(r["to"][n]) == (0xFF if local else frm)
            self.kinds.add((kind, frm == g % N))
            self.answered += 1
        rel = pm.read_released.cpu().numpy()
        assert int(rel.sum()) == count and not rel[~self.is_leader].any()


def test_every_read_is_answered_once_and_to_the_right_node(eng):
    lp = Loop(eng, 8101)
    c_start = lp.committed().copy()
    for rnd in range(12):
        if rnd % 3 == 2:
            lp.propose_round()
        else:
            lp.read_round(0.8, 0.3)
    waiting = len(lp.pending)
    for _ in range(2):  # the network heals: a heartbeat round with no loss answers the rest
        lp.read_round(0.0, 0.0)
    print(f"answered {lp.answered}, waiting before the heal {waiting}, refused (queue full) "
          f"{lp.full}, messages lost {lp.dropped}")
    assert not lp.pending
    assert lp.answered > 2 * C and waiting > 0 and lp.dropped > 0
    assert lp.kinds >= {(_lib.QE_RS_STATE, False), (_lib.QE_RS_STATE, True),
                        (_lib.QE_RS_RESP, False)}
    lead = lp.is_leader
    assert (lp.committed()[lead] > c_start[lead]).sum() > C // 2  # the reads span commit advances
    assert lp.spanned > 0  # ... some were queued before one and released after it
    assert not lp.ps.read_count.cpu().numpy().any()
