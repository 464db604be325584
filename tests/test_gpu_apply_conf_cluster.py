"""Membership changes in the closed loop: the faulty-network cluster simulation
(tests/cluster_sim.py, subclassed here, not edited) with a node added in a
non-lowest slot and later removed, every node applying the committed change
through qe_apply_conf.

Five slots per cluster, node i in slot i (group c * 5 + i, id i + 1).  The
clusters start as voters {1, 2, 3}; node 4 never joins; node 5 is added, in slot
4 -- the slot = node layout the message routing rests on, where qe_confchange's
lowest-untracked rule would put it in slot 3, node 4's -- and later removed.
The run is row "c" of cluster_sim.ROWS (CheckQuorum, log_runs 16) widened to
five slots and six clusters, without compaction: the term-run log carries no
entry types, so the harness keeps, per cluster, which (index, term) is a conf
change, and a snapshot would have to carry the configuration of its own index.

The log of conf changes is the harness's: a change proposed at a leader is the
entry (last_index, term) after qe_propose; a node applies it once its commit
index covers an entry of that index and term; an entry that lost its index to
another term was never committed and is proposed again.  As raft does, a leader
proposes the next change only after it applied the one before.

Checked: the safety invariants of cluster_sim after every round, convergence
of the final members after the heal, every MsgApp / MsgHeartbeat / MsgSnap
addressed to a slot that holds the receiver's own id in the sender's
configuration, and (on the device) the whole resident state against the models
after every call, the untouched groups byte for byte.
"""
import copy

import numpy as np
import pytest

from oracle import confchange_ref as cc
from oracle import orc
from tests import apply_conf_model as acm
from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import snapshot_model as sm

N, MEMBERS0, NEW_ID, NEW_SLOT = 5, 0b00111, 5, 4
P = cs.ROWS["c"].but(N=N, C=6, p_compact=0.0, fault_rounds=110, heal_rounds=30, seed=23)
ROUND_ADD, ROUND_REMOVE = 15, 60
CHANGES = [(cc.ADD_NODE, NEW_ID, NEW_SLOT), (cc.REMOVE_NODE, NEW_ID, acm.ANY_SLOT)]


class MemberWorld(cs.World):
    """Voters {1, 2, 3} in slots 0-2 of five; a configuration per group."""

    def __init__(self, p):
        super().__init__(p)
        self.pb.inc[:] = MEMBERS0      # (in place: the tick model reads these rows)
        self.pb.tracked[:] = MEMBERS0
        for n in self.nodes:
            n.inc = n.tracked = MEMBERS0
        ids = [s + 1 for s in range(p.N)]  # (an untracked slot's id is ignored)
        self.confs = [sm.Conf(p.N, MEMBERS0, 0, 0, ids=ids) for _ in range(p.G)]


def start_changer():
    ch = acm.SlotChanger(N)
    ch.cfg.inc, ch.slots = {1, 2, 3}, {1: 0, 2: 1, 3: 2}
    ch.prs = {i: cc.Progress(1, False) for i in (1, 2, 3)}
    return ch


class Members:
    """qe_apply_conf on the models: tests/apply_conf_model.py on the world's
    rows, then the nodes' and the ConfStates' view of the new configuration."""

    def init_members(self):
        p = self.p
        self.acm = acm.Model(p.G, p.N, goff=p.goff, max_changes=1, pb=self.w.pb)
        self.acm.changers = [start_changer() for _ in range(p.G)]

    def apply_conf(self, records):
        w, p = self.w, self.p
        self.calls["apply_conf"] += 1
        self.acm.leader = [n.state == fm.ST_LEADER for n in w.nodes]
        w.pb.out = np.zeros(p.G, orc.mask_dtype(p.N))  # (no joint configuration here)
        try:
            out = self.acm.apply(records)
            o = self.acm.switch(out)
        finally:
            w.pb.out = None
        for r in out:
            assert r["result"] in (acm.APPLIED, acm.LEADER), r
            g = r["group"] - p.goff
            n = w.nodes[g] = copy.deepcopy(w.nodes[g])
            old = w.confs[g]
            n.inc, n.tracked = r["inc"], r["tracked"]
            ids = list(old.ids)
            for s in range(p.N):
                if r["tracked"] >> s & 1:
                    ids[s] = r["ids"][s]
                elif old.tracked >> s & 1:
                    ids[s] = 0
            w.confs[g] = sm.Conf(p.N, r["inc"], r["out"], r["learner"], r["learners_next"],
                                 tracked=r["tracked"], auto_leave=r["auto_leave"], ids=ids)
            if r["result"] == acm.LEADER:
                w.pull(g)
        return out, o


class ModelMembers(cs.ModelBackend, Members):
    WORLD = MemberWorld

    def __init__(self, p):
        super().__init__(p)
        self.init_members()


class MemberSim(cs.Sim):
    def __init__(self, p, backend):
        super().__init__(p, backend)
        self.log = [[] for _ in range(p.C)]   # per cluster: {index, term, change, lost}
        self.cursor = [0] * p.G               # conf changes of its cluster a node is past
        self.to_new = 0                       # messages a leader addressed to the new node
        self.sw_results = set()

    # ---- no message to a wrong slot ----
    def send(self, cls, frm_g, to_g, term, m):
        p = self.p
        if cls in (cs.F_CLS, cs.S_CLS):
            conf, s = self.w.confs[frm_g], to_g % p.N
            assert conf.tracked >> s & 1 and conf.ids[s] == s + 1, \
                ("a leader's message to a slot that is not the receiver's", frm_g, to_g, conf.ids)
            self.to_new += s == NEW_SLOT
        super().send(cls, frm_g, to_g, term, m)

    # ---- the conf changes ----
    def propose_changes(self):
        p, w = self.p, self.w
        ne = np.zeros(p.G, np.uint32)
        for c in range(p.C):
            live = [e for e in self.log[c] if not e["lost"]]
            k = len(live)
            if k >= len(CHANGES) or self.round_no + 1 < (ROUND_ADD, ROUND_REMOVE)[k]:
                continue
            for g in range(c * p.N, (c + 1) * p.N):
                # (a leader that applied every change before, and not the node to remove)
                if w.nodes[g].state == fm.ST_LEADER and self.past(g) == k and \
                        not (k == 1 and g % p.N == NEW_SLOT):
                    ne[g] = 1
                    break
        if not ne.any():
            return
        self.do_propose(ne)
        for g in np.flatnonzero(ne):
            n, c = w.nodes[g], g // p.N
            k = len([e for e in self.log[c] if not e["lost"]])
            self.log[c].append({"index": n.last_index(), "term": n.term, "change": CHANGES[k],
                                "lost": False})

    def past(self, g):
        """The live changes node g has applied."""
        return len([e for e in self.log[g // self.p.N][: self.cursor[g]] if not e["lost"]])

    def apply_committed(self):
        p, w, st = self.p, self.w, self.p.stride
        while True:
            records, entries = [], []
            for g, n in enumerate(w.nodes):
                log = self.log[g // p.N]
                while self.cursor[g] < len(log):
                    e = log[self.cursor[g]]
                    if n.committed < e["index"]:
                        break
                    if n.log_term(e["index"]) != e["term"]:
                        e["lost"] = True  # another term's entry was committed at its index
                    if e["lost"]:
                        self.cursor[g] += 1
                        continue
                    records.append((p.goff + g, acm.AUTO, 1, [e["change"]]))
                    entries.append(g)
                    break
            if not records:
                return
            nxt0 = w.pb.next.copy()
            out, o = self.be.apply_conf(records)
            for g, r in zip(entries, out):
                self.cursor[g] += 1
                self.cov["conf_applied"] += 1
                if r["result"] == acm.LEADER:
                    self.cov["conf_applied_leader"] += 1
                    self.sw_results.add(r["sw_result"] & 0xF)
                    self.emit(g, int(o.sent[g]), int(o.snap[g]), self.next_index_rule(g, nxt0))

    def round(self):
        self.propose_changes()
        view = super().round()
        self.apply_committed()
        return view

    def run(self):
        p = self.p
        for _ in range(p.fault_rounds + p.heal_rounds):
            self.round()
        view = self.be.view()
        self.inv.check(view)
        self.members_converged(view)
        self.finish(view)
        return self

    def members_converged(self, view):
        """Invariants.converged over the final members: nodes 4 and 5 are no
        members (a removed node may never learn of it: nobody sends to it)."""
        p, w = self.p, self.w
        for c in range(p.C):
            live = [e for e in self.log[c] if not e["lost"]]
            assert len(live) == len(CHANGES), ("not every change was proposed", c, self.log[c])
            vs = view[c * p.N:(c + 1) * p.N]
            members = [s for s in range(p.N) if MEMBERS0 >> s & 1]
            for s in members:
                g = c * p.N + s
                assert self.past(g) == len(CHANGES) and w.confs[g].inc == MEMBERS0 and \
                    w.confs[g].tracked == MEMBERS0 and w.confs[g].ids[NEW_SLOT] == 0, (c, s)
            lead = [s for s in members if vs[s]["state"] == fm.ST_LEADER]
            assert len(lead) == 1 and vs[lead[0]]["term"] == max(vs[s]["term"] for s in members), \
                ("not one leader among the members at their highest term", c, vs)
            ld = vs[lead[0]]
            for s in members:
                v = vs[s]
                lo, hi = max(v["first_index"], ld["first_index"]) - 1, v["last_index"]
                assert v["committed"] == ld["last_index"] == hi and \
                    cs.terms_of(v, lo, hi) == cs.terms_of(ld, lo, hi), (c, s, v, ld)


def check_run(sim):
    assert not sim.cov.get("CP_COMPACTED"), "the run was to have no snapshot"
    assert sim.cov["conf_applied_leader"] >= 2 * P.C           # both changes, at a leader each
    assert sim.cov["conf_applied"] >= (3 * 2 + 1) * P.C        # the members both, the new node its own
    assert sim.to_new > 0 and sim.cov["FR_APP_ACCEPT"] > 0
    assert sim.sw_results <= {3, 4} and sim.sw_results, sim.sw_results  # QE_SW_BCAST / _PROBE


def test_membership_on_the_models():
    sim = MemberSim(P, ModelMembers(P)).run()
    check_run(sim)


@pytest.mark.gpu
def test_membership_on_the_device():
    """The same run with every call on the device too: qe_apply_conf on every
    node that applies a change, the whole resident state compared after it."""
    import torch
    from etcd_amd import engine as eng
    from tests.test_gpu_cluster import DEV, DeviceBackend

    class DeviceMembers(DeviceBackend, Members):
        WORLD = MemberWorld

        def __init__(self, engine, p):
            super().__init__(engine, p)
            self.init_members()

        def apply_conf(self, records):
            e, ps, p = self.e, self.ps, self.p
            m = len(records)
            ac = e.ApplyConf(ps, m, max_changes=1)
            ac.load_host(group=np.array([r[0] for r in records], np.uint64),
                         transition=np.array([r[1] for r in records], np.uint8),
                         num_changes=np.array([r[2] for r in records], np.uint8),
                         type=np.array([[r[3][0][0] for r in records]], np.uint8),
                         node_id=np.array([[r[3][0][1] for r in records]], np.uint64),
                         slot=np.array([[r[3][0][2] for r in records]], np.uint8))
            sw = e.Switch(ps)
            ps.out = self.conf.out  # (the leader half wants the outgoing row: all zero here)
            try:
                self.timed(e.apply_conf, ps, self.fol, self.conf, ac, sw)
            finally:
                ps.out = None
            out, o = Members.apply_conf(self, records)
            touched = np.zeros(p.G, bool)
            touched[[r[0] - p.goff for r in records]] = True
            host = self.after(touched, [sw.result, sw.sent, sw.snap])
            for k, h in zip(("result", "sent", "snap"), host):
                np.testing.assert_array_equal(h, getattr(o, k), err_msg="switch " + k)
            _, rec = ac.records()
            for k in ("result", "cc_result", "sw_result", "inc", "out", "learner", "learners_next",
                      "tracked", "new_progress", "auto_leave"):
                np.testing.assert_array_equal(rec[k].astype(np.int64), [r[k] for r in out],
                                              err_msg=k)
            return out, o

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    ref = MemberSim(P, ModelMembers(P)).run()
    sim = MemberSim(P, DeviceMembers(eng, P)).run()
    check_run(sim)
    assert sim.counters() == ref.counters() and sim.inv.leaders == ref.inv.leaders
    assert DEV.startswith("cuda")
