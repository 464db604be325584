"""tests/cluster_sim.py with duties H4 and H6 (and the QE_TICK_HUP half of H1)
done by qe_inbox's rules: a Sim whose `deliver` turns the queue into a record
list, routes it (tests/inbox_model.py; tests/test_gpu_inbox_cluster.py routes on
the device instead) and drives do_follow / do_snap / do_progress / do_vote from
the rows that come back.  With qe_inbox H4, H6 and H1's HUP are optional for a
host.  `CallLog` records what every step call was given, so a stock run and an
inbox run can be compared call by call.  Imports no torch."""
from collections import Counter

import numpy as np

from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import inbox_model as im
from tests import snapshot_model as sm
from tests import vote_model as vm

F_TYPE = {fm.LMSG_APP: im.APP, fm.LMSG_HEARTBEAT: im.HEARTBEAT}
V_TYPE = {v: k for k, v in im.VMSG.items()}
# the kinds of decision the two rows of tests/test_gpu_inbox_cluster.py must show together
REQUIRED = ("joined", "waves_of_3", "same_slot_close", "class_close", "stepdown", "lower_term",
            "not_leader")
# The reduced row "b" of tests/test_gpu_inbox_cluster.py: 6 clusters of 5, 42
# rounds, seed 3.  Row "c" alone shows one joined response; this one shows the
# response waves (tests/test_inbox_model.py holds what the two must show).
ROW_B_SMALL = dict(C=6, seed=3, fault_rounds=30, heal_rounds=12)
# what each of the two rows shows on the CPU models (their union is REQUIRED)
REQUIRED_BY_ROW = {
    "c": ("joined", "same_slot_close", "class_close", "stepdown", "lower_term", "not_leader"),
    "b_small": ("joined", "waves_of_3", "same_slot_close", "class_close", "not_leader"),
}
assert {k for ks in REQUIRED_BY_ROW.values() for k in ks} == set(REQUIRED)


class CallLog:
    """Mixin for a Sim: `calls_seen` lists (entry point, what it was given)."""

    def log(self, what, x):
        if not hasattr(self, "calls_seen"):
            self.calls_seen = []
        self.calls_seen.append((what, x))

    def do_follow(self, msgs, retried=False):
        self.log("follow", {g: (m.type, m.frm, m.term, m.index, m.log_term, m.commit,
                                tuple(m.runs)) for g, m in enumerate(msgs) if m.type})
        super().do_follow(msgs, retried)

    def do_snap(self, msgs):
        self.log("snap", {g: (m.type, m.frm, m.term, m.sindex, m.sterm, m.inc, m.out, m.learner,
                              m.learners_next, m.auto_leave) for g, m in enumerate(msgs) if m.type})
        super().do_snap(msgs)

    def do_progress(self, items):
        self.log("progress", sorted((g, s, tuple(int(v) for v in m)) for g, s, m in items))
        super().do_progress(items)

    def do_vote(self, msgs):
        self.log("vote", {g: (m.type, m.frm, m.term, m.index, m.log_term, m.flags)
                          for g, m in enumerate(msgs) if m.type})
        super().do_vote(msgs)


class StockSim(CallLog, cs.Sim):
    """The stock simulation, recording its calls."""


class InboxSim(CallLog, cs.Sim):
    """Sim.deliver by qe_inbox's rules.  `kinds` counts the decisions taken;
    `dispositions` the records by disposition."""

    def __init__(self, p, backend, same_from_joins=False, **kw):
        super().__init__(p, backend, **kw)
        assert not self.stale_resp_ok
        self.same_from_joins = same_from_joins
        self.kinds, self.dispositions = Counter(), Counter()

    # ---- a message in flight as a record ----
    def record(self, x):
        g, m = self.p.goff + x.to, x.m
        if x.cls == cs.F_CLS:
            return im.rec(g, x.frm, F_TYPE[m.type], m.term, m.index, m.log_term, m.commit,
                          ents=m.runs)
        if x.cls == cs.S_CLS:
            return im.rec(g, x.frm, im.SNAP, m.term, m.sindex, m.sterm)
        if x.cls == cs.V_CLS:
            return im.rec(g, x.frm, V_TYPE[m.type], m.term, m.index, m.log_term, flags=m.flags)
        t, index, hint, log_term = m
        return im.rec(g, x.frm, t + 3, x.term or 0, index, log_term, hint=hint)  # H11: term 0

    def route(self, recs, tick_action):
        w, p = self.w, self.p
        st = im.state(num_groups=p.G, group_offset=p.goff, num_slots=p.N, stride=p.stride,
                      term=[n.term for n in w.nodes], state=[n.state for n in w.nodes])
        return im.route(st, recs, tick_action, cs.MSG_RUNS, self.same_from_joins)

    def count_kinds(self, recs, out):
        p = self.p
        for g, members in out.waves.items():
            if members[0] == im.SRC_TICK or im.cls_of(recs[members[0]]["type"]) != im.R_CLS:
                continue
            self.kinds["joined"] += len(members) - 1
            self.kinds["waves_of_3"] += len(members) >= 3
            later = [i for i in out.deferred
                     if recs[i]["group"] == p.goff + g and i not in members]
            if later:
                c = im.cls_of(recs[later[0]]["type"])
                self.kinds["same_slot_close" if c == im.R_CLS else "class_close"] += 1
            self.kinds["higher_term_deferred"] += sum(
                out.disposition[i] == im.DEFERRED for i in members)

    def deliver(self, queue):
        p = self.p
        # H1: the HUPs of the tick stand in front (seq 0); they reach qe_inbox as
        # the tick's action row, not as records
        hups = [x for x in queue if x.seq == 0]
        queue = [x for x in queue if x.seq != 0]
        tick_action = None
        if hups:
            tick_action = np.zeros(p.G, np.uint8)
            tick_action[[x.to for x in hups]] = im.TICK_HUP
        self.carry = 0  # the leading records that are the pass before's deferred list
        while queue or tick_action is not None:
            recs = [self.record(x) for x in queue]
            out = self.route(recs, tick_action)
            tick_action = None
            assert all(d in im.ID_NAMES for d in out.disposition), out.disposition
            assert im.BAD not in out.disposition
            self.count_kinds(recs, out)
            for i, d in enumerate(out.disposition):
                self.dispositions[im.ID_NAMES[d]] += 1
                if d == im.DROP_LOWER_TERM:
                    self.discards["resp_lower_term"] += 1
                    self.kinds["lower_term"] += 1
                elif d == im.DROP_NOT_LEADER:
                    local = recs[i]["term"] == 0
                    self.discards["snap_status_not_leader" if local else "resp_not_leader"] += 1
                    self.kinds["not_leader"] += 1
                elif d == im.STEPDOWN:
                    self.cov["resp_higher_term"] += 1
                    self.kinds["stepdown"] += 1
            mark = len(self.net_q)
            if out.f:
                self.do_follow([self.fmsg(out.f.get(g)) for g in range(p.G)])
            if out.s:
                self.do_snap([self.smsg(out.s.get(g), queue) for g in range(p.G)])
            if out.r:  # qe_progress_step before qe_vote_step
                self.do_progress([(g, s, (r["type"], r["index"], r["hint"], r["log_term"]))
                                  for (s, g), r in sorted(out.r.items(), key=lambda kv: kv[1]["src"])])
            if out.v:
                self.do_vote([self.vmsg(out.v.get(g)) for g in range(p.G)])
            new = [x for x in self.net_q[mark:] if x.due <= self.round_no]
            self.net_q[mark:] = [x for x in self.net_q[mark:] if x.due > self.round_no]
            queue = [queue[i] for i in out.deferred] + sorted(self.arrived(new),
                                                              key=lambda x: x.seq)
            self.carry = len(out.deferred)

    @staticmethod
    def fmsg(r):
        if r is None:
            return fm.Msg()
        runs = [e for e in (r["ents"] or ()) if e[0]]
        return fm.Msg(r["type"], r["frm"], r["term"], r["index"], r["log_term"], r["commit"], runs)

    @staticmethod
    def smsg(r, queue):
        """The ConfState is not in a record: the host takes it from the message
        s_src names."""
        if r is None:
            return sm.SMsg()
        m = queue[r["src"]].m
        return sm.SMsg(r["type"], r["frm"], r["term"], r["snap_index"], r["snap_term"], m.inc,
                       m.out, m.learner, m.learners_next, m.auto_leave, m.ids)

    @staticmethod
    def vmsg(r):
        if r is None:
            return vm.Msg()
        return vm.Msg(r["type"], r["frm"], r["term"], r["index"], r["log_term"], r["flags"])
