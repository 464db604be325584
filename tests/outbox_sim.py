"""tests/cluster_sim.py with duty H7 checked against qe_outbox's rules: a
backend that lists, after every leader-side call, the records the call's masks
ask for (tests/outbox_model.py on the World's rows), and a Sim whose `send`
holds every MsgApp / MsgSnap / MsgHeartbeat the host rule builds against the
record for (sender group, slot).  Imports no torch."""
from collections import Counter

import numpy as np

from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import outbox_model as om
from tests import snapshot_model as sm


class OutboxMismatch(AssertionError):
    pass


def world_state(w):
    """The World's rows as qe_progress names them."""
    p, pb = w.p, w.pb
    return om.state(num_groups=p.G, group_offset=p.goff, num_slots=p.N, stride=p.stride,
                    log_runs=p.R, committed=pb.committed, last_index=pb.last_index,
                    run_first=pb.run_first, run_term=pb.run_term, run_count=pb.run_count,
                    next=pb.next, peer=pb.pw, snap_index=pb.snap_index,
                    first_index=pb.first_index)


def by_peer(recs, goff):
    out = {(r["group"] - goff, r["to"]): r for r in recs}
    assert len(out) == len(recs), "two records for one (group, slot)"
    return out


class ModelOutbox(cs.ModelBackend):
    """ModelBackend whose leader-side calls leave the model's records in
    `self.outbox`, {(group, slot): record}; every record of a call must have
    been taken before the next call lists its own."""

    def __init__(self, p, replicate_before=True, **kw):
        super().__init__(p, **kw)
        self.outbox, self.replicate_before = {}, replicate_before

    def list_records(self, **inp):
        if self.outbox:
            raise OutboxMismatch(f"records no message was built for: {self.outbox}")
        term = [n.term for n in self.w.nodes]
        recs, _ = om.build(world_state(self.w), om.inputs(term=term, **inp), cs.MSG_RUNS,
                           self.replicate_before)
        self.outbox = by_peer(recs, self.p.goff)

    def tick(self, events, ticks):
        out = super().tick(events, ticks)
        self.list_records(hb_sent=out.hb_sent, hb_commit=out.hb_commit, hb_ctx=out.hb_ctx)
        return out

    def become_leader(self, elected):
        o = super().become_leader(elected)
        won = o.result == cs.BL_LEADER
        # every peer of a new leader probes: Next is untouched by the send
        self.list_records(sent=np.where(won, o.sent, 0), snap=np.where(won, o.snap, 0),
                          next_before=self.w.pb.next)
        return o

    def propose(self, num_entries):
        nxt0 = self.w.pb.next.copy()
        o = super().propose(num_entries)
        self.list_records(sent=o.sent, snap=o.snap, next_before=nxt0)
        return o

    def progress_step(self, mtype, mindex, mhint, mlogterm):
        o = super().progress_step(mtype, mindex, mhint, mlogterm)
        self.list_records(sent=o.sent, snap=o.snap, index=o.msg_index)
        return o


class OutboxSim(cs.Sim):
    """Sim whose every F-class / S-class message is compared with the backend's
    record for (sender, slot): type, term, index, log_term, commit, runs.  With
    rebuild=True the message that goes on the network is rebuilt from the
    record, so what a follower steps on is what the records say.  `sent_cov`
    counts the kinds of message that went by."""

    def __init__(self, p, backend, rebuild=False, **kw):
        super().__init__(p, backend, **kw)
        self.rebuild, self.sent_cov = rebuild, Counter()

    def send(self, cls, frm_g, to_g, term, m):
        if cls in (cs.F_CLS, cs.S_CLS):
            m = self.check_record(cls, frm_g, to_g % self.p.N, term, m)
        super().send(cls, frm_g, to_g, term, m)

    def check_record(self, cls, g, s, term, m):
        p, w = self.p, self.w
        rec = self.be.outbox.pop((g, s), None)
        if rec is None:
            raise OutboxMismatch(f"no record for the message of group {g} to slot {s}: {vars(m)}")
        frm = g % p.N
        if cls == cs.S_CLS:
            want = dict(type=om.SNAP, index=m.sindex, log_term=m.sterm, commit=0, ents=[])
            new = sm.SMsg(sm.SMSG_SNAP, frm, rec["term"], rec["index"], rec["log_term"], w.inc, 0,
                          w.learner)
            self.sent_cov["snap"] += 1
        elif m.type == fm.LMSG_HEARTBEAT:
            want = dict(type=om.HEARTBEAT, index=0, log_term=0, commit=m.commit, ents=[])
            new = fm.Msg(fm.LMSG_HEARTBEAT, frm, rec["term"], commit=rec["commit"])
            self.sent_cov["heartbeat"] += 1
        else:
            want = dict(type=om.APP, index=m.index, log_term=m.log_term, commit=m.commit,
                        ents=list(m.runs))
            new = fm.Msg(fm.LMSG_APP, frm, rec["term"], rec["index"], rec["log_term"],
                         rec["commit"], rec["ents"])
            n = w.nodes[g]
            after = [t for _, t in n.ents[m.index - n.ents[0][0] + 1:]]
            runs = 1 + sum(a != b for a, b in zip(after, after[1:])) if after else 0
            self.sent_cov["app"] += 1
            self.sent_cov["app_empty"] += runs == 0
            self.sent_cov["app_two_runs"] += len(m.runs) >= 2
            self.sent_cov["app_cut"] += runs > cs.MSG_RUNS
        want.update(term=term, to=s, group=p.goff + g)
        got = {k: rec[k] for k in want}
        got["ents"] = [tuple(e) for e in got["ents"]]
        if got != want:
            raise OutboxMismatch(f"group {g} slot {s}: record {got}, the host rule builds {want}")
        return new if self.rebuild else m

    def run(self):
        super().run()
        if self.be.outbox:
            raise OutboxMismatch(f"records no message was built for: {self.be.outbox}")
        return self


# The reduced row "a" of tests/test_gpu_outbox_cluster.py, chosen on the CPU
# (tests/test_outbox_model.py holds what it must show): 6 clusters, 56 rounds,
# every index still crossing 2^32.  A MsgApp is cut at QE_MAX_MSG_RUNS only when
# more than four term runs follow its Index, which log_runs 4 (the 16-bit
# Inflights form of row "a") rules out: log_runs 8 with 32-bit rings, and an
# election timeout of 2 with longer odds of a cut-off node, so that a follower
# falls five terms behind (seed 2 does; a scan over seeds 1..8 found it).
ROW_A_SMALL = dict(C=6, R=8, ring16=False, ET=2, p_cut=0.3, seed=2, fault_rounds=40,
                   heal_rounds=16)
REQUIRED = ("snap", "app_two_runs", "app_cut", "app_empty", "heartbeat")
