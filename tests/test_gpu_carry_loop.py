"""qe_carry as the transport of the closed loops, on the device.

1. The linearizable-read loop of tests/test_gpu_read_states_loop.py with its
   host hop replaced: every list the leaders and the followers send goes from
   the Outbox / the Replies where it stands through engine.carry into the
   Inbox, with the losses of the same seeded draw; at every hop the Inbox the
   device built equals the one the host builds, field for field.
2. A snapshot exchange on 3-node clusters: qe_compact, qe_progress_send,
   qe_outbox -> qe_carry -> qe_inbox -> qe_snapshot_step / qe_progress_step,
   with one follower of half the clusters cut off.  The MsgSnapStatus the
   leader needs (duty H11) is the one qe_carry made: no host code builds it."""
import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import carry_model as cm
from tests.test_gpu_progress import DEV
from tests.test_gpu_read_states_loop import C as CLUSTERS
from tests.test_gpu_read_states_loop import G, N, Loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def same_list(a, b):
    """Two Inboxes hold the same list, field for field, ent rows included."""
    assert a.n == b.n
    for k in a.RECORD:
        assert torch.equal(getattr(a, k)[:a.n], getattr(b, k)[:b.n]), k
    for k in ("ent_len", "ent_term"):
        assert torch.equal(getattr(a, k)[:a.msg_runs * a.n], getattr(b, k)[:b.msg_runs * b.n]), k


class DeviceLoop(Loop):
    """Loop with the hop on the device: the host-built Inbox stays as the yardstick."""

    def __init__(self, e, seed):
        super().__init__(e, seed)
        self.peers = e.Peers.clusters(self.ps, N)
        self.dib = e.Inbox(self.ps, G * N, 1)
        self.hops = 0

    def carry(self, count, recs, p_drop):
        src = self.rp if "hint" in recs else self.ob   # (a Replies list has hints, an Outbox none)
        state = self.rng.bit_generator.state
        host = super().carry(count, recs, p_drop)
        after = self.rng.bit_generator.state
        self.rng.bit_generator.state = state           # the same draw, once more
        lost = self.rng.random(count) < p_drop
        assert self.rng.bit_generator.state == after
        res = self.e.carry(self.ps, self.peers, src, self.dib, after=0, drop=lost)
        assert (res.n, res.remote_count) == (count, 0) and res.count == count - int(lost.sum())
        disp, _ = res.host()
        assert np.array_equal(disp, np.where(lost, cm.LOST, cm.LOCAL))
        same_list(self.dib, host)
        self.hops += 1
        return self.dib


def test_read_loop_with_the_hop_on_the_device(eng):
    lp = DeviceLoop(eng, 8101)
    c_start = lp.committed().copy()
    for rnd in range(12):
        if rnd % 3 == 2:
            lp.propose_round()
        else:
            lp.read_round(0.8, 0.3)
    waiting = len(lp.pending)
    for _ in range(2):  # the network heals: a heartbeat round with no loss answers the rest
        lp.read_round(0.0, 0.0)
    assert lp.hops == 2 * 14
    # the closing assertions of the host-hop loop
    assert not lp.pending
    assert lp.answered > 2 * CLUSTERS and waiting > 0 and lp.dropped > 0
    assert lp.kinds >= {(_lib.QE_RS_STATE, False), (_lib.QE_RS_STATE, True),
                        (_lib.QE_RS_RESP, False)}
    lead = lp.is_leader
    assert (lp.committed()[lead] > c_start[lead]).sum() > CLUSTERS // 2
    assert lp.spanned > 0
    assert not lp.ps.read_count.cpu().numpy().any()


# ---- 2. the snapshot exchange ----
def cluster_state(e, rng, clusters, S=3, R=4, F=4):
    """The state tests/test_gpu_snapshot.py sets up for its leader-side chain, the three
    nodes of every cluster in ONE batch: node 0 leads at term 1 with the log 1..L all
    committed and its peers in slots 0..2 (slot 2 probing at Next 1), node 1 is in step,
    node 2 has an empty log at term 0."""
    from tests import follower_model as fm
    from tests import snapshot_model as sm

    n_groups = 3 * clusters
    L = np.repeat(rng.integers(4, 40, clusters), 3).astype(np.uint64)
    node = np.arange(n_groups) % 3
    ps = e.ProgressState(n_groups, S, F, R, DEV, extras=("self_slot", "snap_index", "tracked"))
    st = ps.stride
    nodes = [sm.SNode(fm.Node([(0, 0)]), sm.Conf(S), 2, 0) if node[g] == 2 else
             sm.SNode(fm.Node([(0, 0)] + [(i, 1) for i in range(1, int(L[g]) + 1)], int(L[g]), 1,
                              fm.ST_LEADER if node[g] == 0 else fm.ST_FOLLOWER, 0),
                      sm.Conf(S), int(node[g]), 0) for g in range(n_groups)]
    a = sm.pack_snodes(nodes, R, S, st)
    match, nxt = np.zeros((S, st), np.uint64), np.ones((S, st), np.uint64)
    flags = np.zeros((S, st), np.uint8)
    for s in (0, 1):
        match[s, :n_groups], nxt[s, :n_groups] = L, L + 1
        flags[s, :n_groups] = _lib.QE_PR_REPLICATE | _lib.QE_PF_RECENT_ACTIVE
    flags[2, :n_groups] = _lib.QE_PR_PROBE | _lib.QE_PF_RECENT_ACTIVE
    ps.load_host(match=match, next=nxt, flags=flags.reshape(-1),
                 term_start=np.ones(n_groups, np.uint64), tracked=np.full(n_groups, 7, np.uint8),
                 **{k: a[k] for k in ("committed", "last_index", "run_count", "first_index",
                                      "snap_index", "self_slot", "run_first", "run_term")})
    fol = e.Follower(ps)
    fol.load_host(**{k: a[k] for k in ("term", "state", "lead", "vote")})
    cs = e.ConfState(n_groups, S, DEV)
    cs.slot_ids.copy_(torch.from_numpy(a["c_slot_ids"].view(np.int64)).to(DEV))
    for k in sm.CONF_MASKS:
        getattr(cs, k).copy_(torch.from_numpy(a["c_" + k]))
    cs.auto_leave.copy_(torch.from_numpy(a["c_auto_leave"]))
    return ps, fol, cs, L, node


def test_snapshot_exchange_with_the_status_made_on_the_device(eng):
    from tests import snapshot_model as sm

    e, rng = eng, np.random.default_rng(77)
    clusters, S = 47, 3                       # 141 groups: three tiles, the last ragged
    ps, fol, cs, L, node = cluster_state(e, rng, clusters)
    n_groups, st = ps.G, ps.stride
    leader, lagging = node == 0, node == 2
    ci = np.where(leader, [int(rng.integers(1, int(x))) for x in L], 0).astype(np.uint64)
    # the leaders compact and keep a snapshot; their next send to slot 2 is a MsgSnap
    cp = e.Compaction(ps)
    cp.load_host(compact_index=ci, create_index=ci, applied=np.where(leader, L, 0).astype(np.uint64))
    e.compact(ps, cp)
    assert (cp.result.cpu().numpy()[leader] == sm.CP_CREATED | sm.CP_COMPACTED).all()
    before = ps.next.clone()
    want = torch.from_numpy(np.where(leader, 4, 0).astype(np.uint8)).to(DEV)
    sent, snap = e.progress_send(ps, want, send_if_empty=True)
    assert (snap.cpu().numpy() == np.where(leader, 4, 0)).all()
    ob = e.Outbox(ps, n_groups, 1)
    e.outbox(ps, fol.term, ob, sent=sent, snap=snap, next_before=before, snap_term=cp.snap_term)
    count, recs = ob.records()
    assert count == clusters and (recs["type"] == _lib.QE_OMSG_SNAP).all()
    # the link leader -> slot 2 is down in every other cluster
    down = leader & ((np.arange(n_groups) // 3) % 2 == 1)
    cut = np.where(down, 4, 0).astype(np.uint8)
    peers = e.Peers.clusters(ps, 3)
    ib = e.Inbox(ps, 2 * n_groups, 1)
    res = e.carry(ps, peers, ob, ib, cut=cut)
    n_down = int(down.sum())
    assert 0 < n_down < clusters and res.count == 2 * (clusters - n_down) + n_down
    disp, _ = res.host()
    assert sorted(np.unique(disp)) == [cm.LOCAL, cm.LOST] and (disp == cm.LOST).sum() == n_down
    types = ib.type[:ib.n].cpu().numpy()
    assert (types == _lib.QE_IMSG_SNAP_STATUS).sum() == clusters - n_down
    assert (types == _lib.QE_IMSG_SNAP_STATUS_REJECT).sum() == n_down
    # the receivers: the MsgSnap at node 2, the status at the leader's slot 2
    lm, smg, vm, pm = e.LeaderMsgs(ps, 1), e.SnapMsgs(ps, ids=True), e.VoteMsgs(ps), e.PeerMsgs(ps)
    smg.cs_inc.fill_(7)                       # the ConfState is the application's (qe_inbox rule 5)
    smg.load_host(cs_ids=sm.pack_smsgs([sm.SMsg()] * n_groups, S, st)["cs_ids"])
    e.inbox(ps, fol, ib, lm, smg, vm, pm)
    assert not int(ib.deferred_count.item())
    assert (ib.disposition[:ib.n] == _lib.QE_ID_ROUTED).all()
    delivered = lagging & ~np.roll(down, 2)   # node 2 of a cluster whose link is up
    assert np.array_equal(smg.type.cpu().numpy() != 0, delivered)
    rt = pm.type.cpu().numpy().reshape(S, st)[2, :n_groups]
    assert np.array_equal(rt, np.where(down, _lib.QE_MSG_SNAP_STATUS_REJECT,
                                       np.where(leader, _lib.QE_MSG_SNAP_STATUS, 0)))
    out = e.snapshot_step(ps, fol, cs, smg)
    o = out.host()
    assert (o["result"][delivered] == sm.SR_RESTORED).all() and not o["result"][~delivered].any()
    committed = ps.committed.cpu().numpy().view(np.uint64)
    assert np.array_equal(committed[delivered], np.roll(ci, 2)[delivered])
    assert not committed[lagging & ~delivered].any()
    e.progress_step(ps, pm)
    h = ps.host()
    state = (h["flags"].reshape(S, st)[2, :n_groups] & _lib.QE_PF_STATE)[leader]
    assert (state == _lib.QE_PR_PROBE).all()  # both kinds leave StateSnapshot
    assert not h["pending"].reshape(S, st)[2, :n_groups][leader].any()
    nxt = h["next"].reshape(S, st)[2, :n_groups]
    assert np.array_equal(nxt[leader & ~down], ci[leader & ~down] + 1)   # max(Match, PendingSnapshot) + 1
    assert (nxt[down] == 1).all()                                        # Match + 1: the snapshot is resent
